#!/usr/bin/env python3
"""What channel levels + power squelch cost the fused kernel: interleaved pairs of launches at bench.py's default line (256 streams x 16 blocks,
FMD_MATH_FAST, its synthetic FM input) - run_device on one batch, run_device_levels with squelch on on another - for stereo and mono 300 k.
Prints the median and spread of fmd_batch_last_kernel_ms (the fused kernel alone) for each, as one JSON line per mode.

The finish kernel (fmd_levels_kernel, csrc/levels.inc) is not in last_kernel_ms: time it from a run of its own under
    rocprofv3 --kernel-trace --stats -d <dir> -o lv -- python3 tools/levels_cost.py --pairs 5
(its row of the kernel stats), not in the same run as the pairs above."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=30)
    ap.add_argument("--preheat", type=int, default=60, help="launches before the pairs (clock settling, as bench.py --preheat)")
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--modes", default="stereo,mono")
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    args = ap.parse_args()

    import torch
    import rtl_fm_player_amd as R
    from bench import BLOCK_LEN, synth_fm_iq
    dev = torch.device("cuda:0")
    S, B = args.streams, args.blocks
    lines = []
    for mode in args.modes.split(","):
        kw = dict(rate_in=300000, rate_out2=48000, mode=2 if mode == "stereo" else 1)
        cfg = R.wbfm_config(block_len=BLOCK_LEN, math=R.MATH_FAST, **kw)
        iq = synth_fm_iq(torch, dev, S, B * BLOCK_LEN // 2, 2.4e6, True, 1).reshape(-1)
        plain, lv = R.BatchDemod(cfg, S, device=0), R.BatchDemod(cfg, S, device=0)
        lv.set_squelch(np.full(S, 0.05, np.float32), 10)
        pcm = [torch.zeros(S * B * b.pcm_stride, dtype=torch.int16, device=dev) for b in (plain, lv)]
        lens = [torch.zeros(S * B, dtype=torch.int32, device=dev) for _ in range(2)]
        levels = torch.zeros((S, B), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()

        def run(which):
            if which == 0:
                plain.run_device(iq, B, pcm[0], lens[0])
                return plain.last_kernel_ms()
            lv.run_device_levels(iq, B, pcm[1], lens[1], levels)
            return lv.last_kernel_ms()

        for i in range(args.preheat):
            run(i & 1)
        t = [[], []]
        for i in range(args.pairs):
            for which in ((0, 1) if i % 2 == 0 else (1, 0)):       # alternate the order inside a pair
                t[which].append(run(which))
        lv.sync()
        st = []
        for v in t:
            a = np.array(v)
            st.append(dict(median_ms=float(np.median(a)), min_ms=float(a.min()), max_ms=float(a.max()),
                           p10_ms=float(np.percentile(a, 10)), p90_ms=float(np.percentile(a, 90))))
        d = np.array(t[1]) - np.array(t[0])
        line = dict(mode=mode, streams=S, blocks=B, math="fast", family=plain.math, pairs=args.pairs, run_device=st[0],
                    run_device_levels_squelch=st[1], cost_median_pct=100.0 * (st[1]["median_ms"] / st[0]["median_ms"] - 1.0),
                    pair_diff_median_ms=float(np.median(d)), pair_diff_p10_ms=float(np.percentile(d, 10)),
                    pair_diff_p90_ms=float(np.percentile(d, 90)), closed_blocks=int((lens[1] == 0).sum()))
        print(json.dumps(line), flush=True)
        lines.append(line)
        plain.close()
        lv.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
