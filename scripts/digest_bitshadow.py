#!/usr/bin/env python3
"""A sha256 (its first 12 hex digits) per output tensor of every entry of the bit-shadow family (pointer.hip, critic.hip,
encode.hip) on tiny seeded shapes, as JSON, a line per launch with the tensors' names in its key: two trees that print the
same file write the same bytes.  B = 5; (Hd, rows, nR) = (64, 30, 20) HPL 1, (128, 30, 40) HPL 2 with two passes of the
backward's dU tile, (128, 70, 20) two planes, (256, 30, 20) two chunks; S = 1 .. 5; the pointer's proj, static-rows, GREEDY
and DRAW forms with their backwards; the critic with 1 and 3 blocks and q0 of stride 0 and H; the encoder.  Uses only names
that the wrappers have kept (``_scores_into`` & co. and the public functions).  Usage:

    python scripts/digest_bitshadow.py [--out profiles/bitshadow_digest.json]
"""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tap_net_amd as T  # noqa: E402,F401
from tap_net_amd import pack, rollout as R  # noqa: E402

B = 5
SHAPES = [(64, 30, 20), (128, 30, 40), (128, 70, 20), (256, 30, 20)]


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:12]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bitshadow_digest.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(20)
    rnd = lambda *s, scale=0.3: (torch.randn(*s, generator=gen) * scale).to(dev)                                 # noqa: E731
    leaf = lambda *s: rnd(*s).requires_grad_()                                                                 # noqa: E731
    out = {}

    def put(key, names, tensors):
        out["%s: %s" % (key, " ".join(names))] = [sha(t) for t in tensors]

    def grads(y, leaves):
        return torch.autograd.grad(y, leaves, rnd(*y.shape, scale=1.0))

    pack.set_binary_check('trust')
    for Hd, rows, nR in SHAPES:
        dyn = (torch.rand(B, rows, nR, generator=gen) < 0.15).float().to(dev)
        bits = pack.dynamic_bits(dyn)[0]
        mask = (torch.rand(B, nR, generator=gen) < 0.7).float().to(dev)
        state = torch.tensor([1234, 5], dtype=torch.int64, device=dev)
        shape = "Hd%d_rows%d_nR%d" % (Hd, rows, nR)
        # the pointer's proj form
        proj, M, k, q, va, vp = leaf(B, 3, nR, Hd), leaf(3 * Hd, rows), leaf(3 * Hd), leaf(B, Hd), leaf(Hd), leaf(Hd)
        bufs = tuple(torch.empty(*s, device=dev) for s in ((B, nR), (B, nR), (B, Hd)))
        with torch.no_grad():
            R._scores_into(proj, bits, M, k, q, va, vp, rows, *bufs)
        put(shape + "/proj", ("logits", "attn", "t"), bufs)
        leaves = (proj, M, k, q, va, vp)
        put(shape + "/proj_bw", ("dU", "dM", "dk", "dq", "dva", "dvp"), grads(R.pointer_scores(proj, bits, M, k, q, va, vp), leaves))
        # the encoder, forward and backward
        w, b = leaf(Hd, rows), leaf(Hd)
        h = R.encode_dynamic_bits(bits, w, b)
        put(shape + "/encode", ("out", "dweight", "dbias"), (h,) + grads(h, (w, b)))
        for S in range(1, 6):
            key = "%s/S%d" % (shape, S)
            xs, G, g = rnd(B, S, nR, scale=1.0), leaf(3 * Hd, S), leaf(3 * Hd)
            with torch.no_grad():
                R._scores_static_into(xs, bits, G, g, M, k, q, va, vp, rows, *bufs)
            put(key + "/static", ("logits", "attn", "t"), bufs)
            leaves = (G, g, M, k, q, va, vp)
            put(key + "/static_bw", ("dG", "dg", "dM", "dk", "dq", "dva", "dvp"),
                grads(R.pointer_scores_static(xs, bits, G, g, M, k, q, va, vp), leaves))
            with torch.no_grad():
                put(key + "/greedy", ("ptr", "logp", "logits"),
                    R.pointer_pick_static(xs, bits, G, g, M, k, q, va, vp, mask, want_logits=True))
                put(key + "/draw", ("ptr", "logp", "logits"),
                    R.pointer_pick_static(xs, bits, G, g, M, k, q, va, vp, mask, source=(state, 3), want_logits=True))
            # the critic: H = Hd, its own folded weights
            cG, cg, cM, v, w2, b2 = leaf(3 * Hd, S), leaf(3 * Hd), leaf(Hd, rows), leaf(Hd), leaf(Hd), leaf(1)
            for blocks in (1, 3):
                for q0 in (leaf(1, Hd), leaf(B, Hd)):
                    ck = "%s/critic_n%d_q0s%d" % (key, blocks, 0 if q0.shape[0] == 1 else Hd)
                    cb = R._critic_buffers(B, S, nR, Hd, blocks, dev)
                    with torch.no_grad():
                        R._critic_into(xs, bits, cG, cg, cM, q0, v, w2, b2, blocks, rows, *cb)
                    put(ck, ("value", "z", "p", "xbar", "q"), cb)
                    leaves = (cG, cg, cM, q0, v, w2, b2)
                    put(ck + "_bw", ("dG", "dg", "dM", "dq0", "dv", "dw2", "db2"),
                        grads(R.critic_value(xs, bits, cG, cg, cM, q0, v, w2, b2, blocks), leaves))
    torch.cuda.synchronize()
    with open(args.out, "w") as f:
        f.write("{\n%s\n}\n" % ",\n".join("%s: %s" % (json.dumps(k), json.dumps(out[k])) for k in sorted(out)))
    print("%d digests -> %s" % (sum(len(v) for v in out.values()), args.out))


if __name__ == "__main__":
    main()
