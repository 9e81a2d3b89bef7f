#!/usr/bin/env python3
"""Time of the station finder (fmd_scan_run_device, csrc/scan.inc) behind the capture spectrum at the bench's shape: 256 streams x 16 blocks x
262144 bytes of IQ on the device (a 32 KiB capture of three FM carriers, noise and a DC offset, tiled: tests/scan_model.capture_bytes), Hann
window, N = 1024 and 4096; raster and bw 100 kHz at 2.4 Msps (21 candidates), dc_guard 2, 16 stations.

HIP events (torch.cuda.Event) on the launch stream around every launch; warm-up launches, then the median of --reps launches with p10 / p90.  Per N,
from the same session: the spectrum call that produced d_power, a device-to-device copy of the same d_power (n_streams x n_blocks x n_bins floats:
what a host-side scanner would have to move at the least), and the scan; the scan's read of d_power as bytes/s.  One JSON line per measurement;
--out also writes them to a file.  The tool ends itself after --timeout seconds; run it on an idle device, and under a timeout of the caller's too:

    timeout -k 10 300 python3 tools/scan_time.py --out profiles/<name>.json"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--block-len", type=int, default=262144)
    ap.add_argument("--bins", default="1024,4096")
    ap.add_argument("--raster", type=int, default=100000)
    ap.add_argument("--bw", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=30, help="timed launches per measurement (>= 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=240, help="seconds after which the tool ends itself (SIGALRM), whatever it is waiting for")
    args = ap.parse_args()
    import signal
    signal.alarm(args.timeout)
    if args.reps < 20:
        ap.error("--reps must be at least 20")

    import torch
    import rtl_fm_player_amd as R
    import scan_model as M
    dev = torch.device("cuda:0")
    S, B, BL = args.streams, args.blocks, args.block_len
    cap = torch.from_numpy(np.array(M.capture_bytes())).to(dev)
    iq = cap.repeat((S * B * BL + cap.numel() - 1) // cap.numel())[:S * B * BL].contiguous()
    b = R.BatchDemod(R.wbfm_config(block_len=BL, rate_in=M.CAPTURE_RATE // 8, rate_out2=48000, mode=2), S, device=0)
    st = torch.cuda.Stream()
    lines = []

    def timed(fn):
        with torch.cuda.stream(st):
            for _ in range(args.warmup):
                fn()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
            for e0, e1 in ev:
                e0.record(st)
                fn()
                e1.record(st)
        st.synchronize()
        t = np.array([e0.elapsed_time(e1) for e0, e1 in ev])
        return dict(median_ms=float(np.median(t)), min_ms=float(t.min()), p10_ms=float(np.percentile(t, 10)),
                    p90_ms=float(np.percentile(t, 90)), max_ms=float(t.max()), reps=args.reps)

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    for n_bins in [int(x) for x in args.bins.split(",")]:
        power = torch.zeros((S, B, n_bins), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        t = timed(lambda: b.spectrum_device(iq, B, n_bins, power, window=R.WINDOW_HANN, hip_stream=st.cuda_stream))
        spectrum_ms = t["median_ms"]
        emit(dict(what="spectrum", n_bins=n_bins, streams=S, blocks=B, block_len=BL, iq_bytes=iq.numel(), **t))
        copy_dst = torch.empty_like(power)
        t = timed(lambda: copy_dst.copy_(power, non_blocking=True))
        copy_ms = t["median_ms"]
        emit(dict(what="d2d_copy_of_d_power", n_bins=n_bins, bytes=power.numel() * 4, bytes_per_s=power.numel() * 4 / (copy_ms * 1e-3), **t))
        del copy_dst
        cfg = R.FmdScanConfig(M.CAPTURE_RATE, n_bins, args.raster, args.bw, 1, 250, 2, 16, 4.0)
        scan = R.Scan(cfg, S, device=0)
        d_st = torch.zeros((S, 16 * 32), dtype=torch.uint8, device=dev)
        d_cnt = torch.zeros((S, 2), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        t = timed(lambda: scan.run_device(power, B, d_st, d_cnt, hip_stream=st.cuda_stream))
        scan.sync()
        off = d_st[0].cpu().numpy().view(M.STATION_DTYPE)["offset_hz"][:int(d_cnt[0, 1])]
        emit(dict(what="scan", n_bins=n_bins, offsets_of_stream_0=[int(x) for x in off], streams=S, blocks=B, candidates=scan.n_candidates, power_bytes=power.numel() * 4,
                  power_bytes_per_s=power.numel() * 4 / (t["median_ms"] * 1e-3), ratio_to_spectrum=t["median_ms"] / spectrum_ms,
                  ratio_to_copy_of_d_power=t["median_ms"] / copy_ms, found=[int(x) for x in d_cnt[:, 0].unique().cpu()], **t))
        scan.close()
        del power, d_st, d_cnt
        torch.cuda.empty_cache()
    b.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
