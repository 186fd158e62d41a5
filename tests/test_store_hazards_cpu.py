"""Store-data hazards in the gfx950 code objects: a VMEM store of more than 8 bytes (dwordx3 / dwordx4) reads its data
VGPRs AFTER it issues, and on gfx940+ a VALU instruction that writes one of them within the next 2 wait states changes
what is stored.  The compiler pads the stores it emits itself; it does not look inside inline assembly
(tap_masks.h: store_stream, probe.hip), where a register allocation once put a loop counter in a write-through store's
data register.  This test disassembles every unit of libtapenv and checks every such store, compiler-emitted or not.

Each csrc/*.hip is taken from the library build (tap-net_amd/csrc/build/<unit>.o, when it is newer than every source
and header) or compiled device-only with the Makefile's flags; its gfx950 code object is unbundled with
clang-offload-bundler and disassembled with ROCm's llvm-objdump.  No GPU needed.  With the library built this takes a few
seconds; without it the 14 device-only compiles take about two minutes on 8 cores.

Limit: the scan follows program order.  A store followed by a branch is checked against the instructions after the
branch, not against those at its target; the stores of the stream waves (store_stream) sit inside their loops' bodies."""
import concurrent.futures
import glob
import os
import re
import shutil
import subprocess
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tap-net_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HIPCC = os.path.join(ROCM, "bin", "hipcc")
BUNDLER = os.path.join(ROCM, "llvm", "bin", "clang-offload-bundler")
OBJDUMP = os.path.join(ROCM, "llvm", "bin", "llvm-objdump")
OBJCOPY = os.path.join(ROCM, "llvm", "bin", "llvm-objcopy")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"

WAIT_STATES = 2      # VMEM store > 8 bytes -> VALU write of its data: 2 wait states on gfx940+ (1 before)

# a VMEM store with 12 or 16 bytes of data, and where its data operand sits: buffer_* puts it first, the others second
STORE = re.compile(r"^(global|buffer|flat|scratch)_store_(dwordx3|dwordx4|b96|b128)\b")
REG = re.compile(r"^([va])(?:(\d+)|\[(\d+):(\d+)\])$")
ADDR = re.compile(r"//\s*([0-9A-Fa-f]+):")
FUNC = re.compile(r"^[0-9a-fA-F]+ <(.+)>:$")


def _regs(op):
    """'v[18:21]' -> ('v', {18, 19, 20, 21}); 'v7' -> ('v', {7}); anything else -> None."""
    m = REG.match(op.strip())
    if not m:
        return None
    if m.group(2) is not None:
        return m.group(1), {int(m.group(2))}
    return m.group(1), set(range(int(m.group(3)), int(m.group(4)) + 1))


def _split(line):
    """One disassembly line -> (mnemonic, operands, offset) or None for labels / blank lines."""
    code, _, comment = line.partition("//")
    code = code.strip()
    if not code or code.endswith(">:"):
        return None
    mnem, _, rest = code.partition(" ")
    ops = [o.strip() for o in rest.split(",")] if rest.strip() else []
    m = ADDR.search(line)
    return mnem, ops, (int(m.group(1), 16) if m else -1)


def _wait_states(mnem, ops):
    if mnem == "s_nop":
        return int(ops[0], 0) + 1 if ops else 1
    return 1


def find_hazards(text):
    """Every store of more than 8 bytes followed, within WAIT_STATES wait states in program order, by a VALU
    instruction that writes one of its data registers -> [(kernel, offset, store, offender)]."""
    out, func, insts = [], "?", []
    for line in text.splitlines():
        m = FUNC.match(line.strip())
        if m:
            func = m.group(1)
            continue
        p = _split(line)
        if p:
            insts.append((func, line.strip(), p))
    for i, (func, line, (mnem, ops, off)) in enumerate(insts):
        if not STORE.match(mnem):
            continue
        data = _regs(ops[0] if mnem.startswith("buffer_") else ops[1])
        assert data is not None, "cannot read the data operand of: " + line
        ws = 0
        for f2, line2, (mnem2, ops2, _) in insts[i + 1:]:
            if ws >= WAIT_STATES or f2 != func:
                break
            if mnem2.startswith("v_") and ops2:
                dst = _regs(ops2[0])
                if dst and dst[0] == data[0] and dst[1] & data[1]:
                    out.append((func, off, line.split("//")[0].strip(), line2.split("//")[0].strip()))
                    break
            ws += _wait_states(mnem2, ops2)
    return out


def count_stores(text):
    return sum(1 for line in text.splitlines() if (p := _split(line)) and STORE.match(p[0]))


# ---- the parser on committed text: one padded store, one unpadded -------------------------------------------------
FIXTURE = """
0000000000001000 <_Z4goodPf>:
\tglobal_store_dwordx4 v[28:29], v[18:21], off sc0 sc1         // 000000001000: DE7D8000 007F121C
\ts_nop 1                                                      // 000000001008: BF800001
\tv_mov_b32_e32 v18, 0                                         // 00000000100C: 7E240280
\tglobal_store_dwordx4 v[2:3], v[4:7], off                     // 000000001010: DC7C8000 007F0402
\tv_add_u32_e32 v8, 4, v8                                      // 000000001018: 68101084
\tbuffer_store_dwordx4 v[10:13], v1, s[0:3], 0 offen           // 00000000101C: E07C1000 80000A01
\ts_waitcnt vmcnt(0)                                           // 000000001024: BF8C0F70
\ts_waitcnt lgkmcnt(0)                                         // 000000001028: BF8CC07F
\tv_mov_b32_e32 v10, 0                                         // 00000000102C: 7E140280
\ts_endpgm                                                     // 000000001030: BF810000

0000000000001100 <_Z3badPf>:
\tglobal_store_dwordx4 v[28:29], v[18:21], off sc0 sc1         // 000000001100: DE7D8000 007F121C
\tv_mov_b32_e32 v18, 0                                         // 000000001108: 7E240280
\ts_endpgm                                                     // 00000000110C: BF810000
"""


def test_parser_flags_only_the_unpadded_store():
    bad = find_hazards(FIXTURE)
    assert bad == [("_Z3badPf", 0x1100, "global_store_dwordx4 v[28:29], v[18:21], off sc0 sc1", "v_mov_b32_e32 v18, 0")]
    assert count_stores(FIXTURE) == 4
    # one wait state of padding is not enough on gfx950
    assert len(find_hazards(FIXTURE.replace("\tv_mov_b32_e32 v18, 0                                         // 000000001108",
                                            "\ts_nop 0\n\tv_mov_b32_e32 v18, 0 // 000000001108"))) == 1


# ---- the code objects ------------------------------------------------------------------------------------------------
def _make_flags():
    """CXXFLAGS and each unit's additions, read from the Makefile."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    base = re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", text, re.M).group(1).split()
    extra = {m.group(1): m.group(2).split() for m in re.finditer(r"^build/(\w+)\.o:\s*CXXFLAGS\s*\+=\s*(.*)$", text, re.M)}
    return base, extra


def _fresh_build(unit):
    """build/<unit>.o when it is newer than every source and header it may depend on, else None."""
    obj = os.path.join(CSRC, "build", unit + ".o")
    if not os.path.exists(obj):
        return None
    deps = glob.glob(os.path.join(CSRC, "*.h")) + [os.path.join(CSRC, unit + ".hip"), os.path.join(ROOT, "include", "tapenv.h"),
                                                    os.path.join(CSRC, "Makefile")]
    return obj if os.path.getmtime(obj) > max(os.path.getmtime(d) for d in deps) else None


def _disassemble(unit, tmp, base, extra):
    bundle = os.path.join(tmp, unit + ".bundle")
    obj = _fresh_build(unit)
    if obj:
        subprocess.check_call([OBJCOPY, "--dump-section=.hip_fatbin=" + bundle, obj, os.path.join(tmp, unit + ".host")])
    else:
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", *base, *extra.get(unit, []), "-I" + os.path.join(ROOT, "include"),
                               "-I" + CSRC, "--cuda-device-only", "-c", os.path.join(CSRC, unit + ".hip"), "-o", bundle])
    co = os.path.join(tmp, unit + ".co")
    subprocess.check_call([BUNDLER, "--type=o", "--targets=" + TARGET, "--input=" + bundle, "--output=" + co, "--unbundle"])
    text = subprocess.run([OBJDUMP, "-d", "--mcpu=gfx950", co], check=True, capture_output=True, text=True).stdout
    return unit, text, bool(obj)


@pytest.fixture(scope="module")
def disassembly(tmp_path_factory):
    for tool in (HIPCC, BUNDLER, OBJDUMP, OBJCOPY):
        if not os.path.exists(tool):
            pytest.skip("ROCm toolchain not found: " + tool)
    tmp = str(tmp_path_factory.mktemp("hazards"))
    base, extra = _make_flags()
    units = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(CSRC, "*.hip")))
    t0 = time.time()
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        res = list(ex.map(lambda u: _disassemble(u, tmp, base, extra), units))
    print("disassembled %d units in %.1f s (%d from the library build)" % (len(res), time.time() - t0, sum(r[2] for r in res)))
    return {u: text for u, text, _ in res}


def test_every_unit_disassembled(disassembly):
    units = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(CSRC, "*.hip")))
    assert sorted(disassembly) == units
    for u, text in disassembly.items():
        assert re.search(r"^[0-9a-f]+ <.+>:$", text, re.M), u
    # the write-through store of the stream waves is there to be checked
    assert re.search(r"global_store_dwordx4 .* sc0 sc1", disassembly["transition"])


def test_no_store_data_hazards(disassembly):
    bad, stores = [], 0
    for u in sorted(disassembly):
        stores += count_stores(disassembly[u])
        bad += [(u,) + h for h in find_hazards(disassembly[u])]
    assert stores > 1000
    assert not bad, "%d store(s) whose data a VALU overwrites within %d wait states:\n%s" % (
        len(bad), WAIT_STATES, "\n".join("%s  %s  +0x%x  %s  ->  %s" % b for b in bad[:40]))
