#!/usr/bin/env python3
"""A/B of the convolution with m input ciphertexts on one GPU, at `conv 3 3`'s shape (B = 256 output channels, one ciphertext of 256 input channels per member):

  (a) the composition a caller had before the grouping rule: ONE hc_conv_then_pack_batch of m members with distinct outputs (m pack trees), then 2(m-1) hc_add of the
      m results - timed on a build of the PARENT commit (--parent-lib; without it this build's library runs side (a) too, and the record says so);
  (b) the grouped call of this build: the m members name one ct_out, the products are summed at level 1, ONE pack tree.

The two sides alternate, round after round, in one process on one device. A figure = --warmup untimed and --steps timed steps between HIP events (hc_timer_start / stop),
as bench.py times its steps. Prints one JSON line: per m the per-round and median ms per step of both sides, the ratio b/a, and the per-kernel totals (hc_profile_get) of
one profiled step of each side.
Usage: tools/multiconv_ab.py [--parent-lib PATH] [--m 2 4] [--B 256] [--steps 20] [--warmup 5] [--rounds 3]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

S30 = 2.0 ** 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libhconv.so built from the parent commit (side a)")
    ap.add_argument("--m", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import parity_cases as pc
    from optimal_conv_amd import Context
    from oracle_lib import P0, Q0, Q1
    N, B = pc.N, a.B
    rng = np.random.default_rng(2025)
    res = rng.integers  # uniform residues: the kernels' time does not depend on the data
    ctx_b = Context([Q0, Q1], [P0], device=0)
    ctx_a = Context([Q0, Q1], [P0], device=0, lib_path=a.parent_lib) if a.parent_lib else ctx_b
    out = {"shape": {"B": B, "k": 3, "N": N}, "steps": a.steps, "warmup": a.warmup, "side_a_library": "parent" if a.parent_lib else "this build", "cases": {}}
    for ctx in {id(ctx_a): ctx_a, id(ctx_b): ctx_b}.values():
        pc.load_tree_keys(ctx, 0xAB, B)
        ctx.idx_load(None)
    for m in a.m:
        ct = [np.stack([np.stack([res(0, q, N, dtype=np.uint64) for q in (Q0, Q1)]) for _ in range(2)]) for _ in range(m)]
        ker = [np.stack([np.stack([res(0, q, N, dtype=np.uint64) for q in (Q0, Q1)]) for _ in range(B)]) for _ in range(m)]
        bias = res(0, Q0, N, dtype=np.uint64)

        def side(ctx):
            return {"ctx": ctx, "in": [ctx.buf(x) for x in ct], "ker": [ctx.ker_load(k) for k in ker], "bias": ctx.buf(bias), "out": [ctx.buf(nwords=2 * N) for _ in range(m)]}
        A, Bs = side(ctx_a), side(ctx_b)

        def step_a():
            c = A["ctx"]
            c.conv_then_pack_batch_dev(A["in"], S30, A["ker"], S30, B, 1, S30, [A["bias"]] + [None] * (m - 1), A["out"])
            o0 = A["out"][0]
            for z in range(1, m):
                for p in range(2):
                    c._ck(c.L.hc_add(c.h, 0, o0.at(p * N), A["out"][z].at(p * N), o0.at(p * N), 1))

        def step_b():
            Bs["ctx"].conv_then_pack_multi_dev([(Bs["in"], Bs["ker"], Bs["bias"], Bs["out"][0])], S30, S30, B, 1, S30)

        def figure(ctx, step):
            for _ in range(a.warmup):
                step()
            ctx.sync()
            ctx.timer_start()
            for _ in range(a.steps):
                step()
            return ctx.timer_stop() / a.steps

        def kernels(ctx, step):
            ctx.set_option("profile", 1)
            ctx.profile_reset()
            step()
            ctx.sync()
            prof = ctx.profile()
            ctx.set_option("profile", 0)
            return {k: {"ms": round(v[0], 4), "launches": v[1]} for k, v in sorted(prof.items())}
        ta, tb = [], []
        for _ in range(a.rounds):
            ta.append(figure(ctx_a, step_a))
            tb.append(figure(ctx_b, step_b))
        ma, mb = float(np.median(ta)), float(np.median(tb))
        out["cases"][f"m={m}"] = {"a_ms": [round(t, 4) for t in ta], "b_ms": [round(t, 4) for t in tb], "a_median_ms": round(ma, 4), "b_median_ms": round(mb, 4),
                                  "b_over_a": round(mb / ma, 4), "a_kernels": kernels(ctx_a, step_a), "b_kernels": kernels(ctx_b, step_b)}
        for S in (A, Bs):
            for b in S["in"] + S["out"] + [S["bias"]]:
                b.free()
            for h in S["ker"]:
                S["ctx"].ker_free(h)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
