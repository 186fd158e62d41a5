"""The host-side mirror (PACKDataset, file format, directory names, RollingDataset) against the reference's results.

The reference's side is recorded in tests/golden/host_reference.npz (tests/golden/make_golden.py --only
host_reference runs the reference over exactly the cases listed here, on the same dataset directories)."""
import os

import numpy as np
import pytest
import torch

import golden_util as G
import tap_net_amd as T
from tap_net_amd import datafiles

INPUT_TYPES = [("bot", True), ("bot", False), ("simple", False), ("rot", True), ("bot-rot", True), ("mul", True),
               ("mul-with", True), ("rot-old", True)]
DIR_NAME_CASES = [(D, n, tr, va, iw, sr) for D in (2, 3)
                  for n, tr, va, iw, sr in ((10, 1000, 100, 7, [1, 5]), (20, 64, 8, 5, [2, 6]))]
ROLLING_INSTANCES = 6


def write_dirs(make_dir):
    """D -> (dataset directory, a second one with the samples reversed for mix_data_file, N); make_dir(name) -> path."""
    out = {}
    for D, N in ((2, 256), (3, 64)):
        z = G.load("dataset_%dd.npz" % D)
        pos = z["txt_pos"].reshape(N, D, 10).transpose(0, 2, 1)
        d = str(make_dir("ds%d" % D)) + "/"
        datafiles.write_dataset(d, z["static"], z["dynamic"], pos, container_ids=z["txt_container"])
        d2 = str(make_dir("mix%d" % D)) + "/"
        datafiles.write_dataset(d2, z["static"][::-1], z["dynamic"][::-1], pos[::-1], container_ids=z["txt_container"][::-1])
        out[D] = (d, d2, N)
    return out


def packdataset_key(D, input_type, allow_rot, hm_type, mix):
    return "packdataset|%d|%s|%s|%s|%s" % (D, input_type, allow_rot, hm_type, mix)


def make_dataset_dirs(D, n, tr, va, iw, sr):
    """The directories create_dataset / create_dataset_gt / get_mix_dataset look for, made in the current directory."""
    for kind in ("rand", "gt"):
        for split, size in (("train", tr), ("valid", va)):
            d = "./data/%s_%dd/pack-%s-%d-%d-%d-%d-%d/" % (kind, D, split, n, size, iw, sr[0], sr[1])
            os.makedirs(d, exist_ok=True)
            with open(d + "blocks.txt", "w") as f:
                f.write("0\n")


def dataset_names(pack, D, n, tr, va, iw, sr):
    """What the three dataset functions return when their directories exist."""
    return [pack.create_dataset(n, tr, va, D, iw, 50, 1, sr, seed=3),
            pack.create_dataset_gt(n, tr, va, D, 5, 50, iw, 50, "bot", 1, sr, seed=3),
            pack.get_mix_dataset(n, tr, va, D, iw, sr, seed=3)]


@pytest.fixture(scope="module")
def rec():
    return G.load("host_reference.npz")


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    return write_dirs(tmp_path_factory.mktemp)


def _want(rec, key):
    k = G.key_index(rec, key)
    pre = "k%d_" % k
    return {f[len(pre):]: rec[f] for f in rec.files if f.startswith(pre)}


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("input_type,allow_rot", INPUT_TYPES)
def test_packdataset_matches_reference(rec, dirs, D, input_type, allow_rot):
    d, d2, N = dirs[D]
    for hm_type in ("diff", "full"):
        for mix in (None, d2):
            want = _want(rec, packdataset_key(D, input_type, allow_rot, hm_type, mix is not None))
            if "error" in want:         # e.g. 'bot' without rotations: the reference cannot build it either
                with pytest.raises(Exception) as e:
                    T.PACKDataset(d, 10, N, 7, input_type, hm_type, allow_rot, 5, mix_data_file=mix, unit=1)
                assert type(e.value).__name__ == str(want["error"])
                continue
            mine = T.PACKDataset(d, 10, N, 7, input_type, hm_type, allow_rot, 5, mix_data_file=mix, unit=1)
            ctx = (input_type, allow_rot, hm_type, mix is not None)
            assert torch.equal(torch.from_numpy(want["static"]), mine.static), ctx
            assert torch.equal(torch.from_numpy(want["dynamic"]), mine.dynamic), ctx
            assert tuple(want["decoder_static_shape"]) == tuple(mine.decoder_static.shape)
            assert tuple(want["decoder_dynamic_shape"]) == tuple(mine.decoder_dynamic.shape)
            assert int(want["len"]) == len(mine)
            item = mine[5]
            assert len(item) == int(want["item5_len"])
            for j, b in enumerate(item):
                assert torch.equal(torch.from_numpy(want["item5_%d" % j]), b)


def test_no_precedence_and_unit(rec, dirs):
    d, _, N = dirs[2]
    want = _want(rec, "no_precedence_unit")
    mine = T.PACKDataset(d, 10, N, 3, "bot", "diff", True, 5, unit=0.5, no_precedence=True)
    assert torch.equal(torch.from_numpy(want["static"]), mine.static)
    assert torch.equal(torch.from_numpy(want["dynamic"]), mine.dynamic)
    assert tuple(want["decoder_dynamic_shape"]) == tuple(mine.decoder_dynamic.shape)


def test_dataset_directory_names_match_reference(rec, tmp_path, monkeypatch):
    """create_dataset / create_dataset_gt / get_mix_dataset name their directories as the reference does
    (pack.py:475-505, 568-608): with the directories already present both sides return without generating."""
    from tap_net_amd import pack as tpack
    monkeypatch.chdir(tmp_path)
    want = [str(x) for x in rec["dir_names"]]
    got = []
    for case in DIR_NAME_CASES:
        make_dataset_dirs(*case)
        got += [repr(x) for x in dataset_names(tpack, *case)]
    assert got == want


@pytest.mark.parametrize("D", [2, 3])
def test_rolling_dataset_reads_what_the_reference_reads(rec, dirs, D):
    """rolling.RollingDataset (rolling.py:462-536): the blocks / positions our reader hands to RollingWindows are
    the arrays the reference hands to each InitialContainer, and the zero decoder inputs have its shapes."""
    from tap_net_amd.rolling import RollingDataset
    d, _, N = dirs[D]
    want = _want(rec, "rolling|%d" % D)
    blocks, positions = RollingDataset.read_instances(d, 10, D, ROLLING_INSTANCES)
    for i in range(ROLLING_INSTANCES):
        assert np.array_equal(want["blocks"][i], blocks[i]) and np.array_equal(want["positions"][i], positions[i])
    assert tuple(want["decoder_static_shape"]) == (1, D, 1)
    assert tuple(want["decoder_dynamic_shape"]) == ((1, 4, 1) if D == 2 else (1, 2, 5, 5))
