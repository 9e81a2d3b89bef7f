#!/usr/bin/env python3
"""Time of the capture spectrum (fmd_batch_spectrum_device, csrc/spectrum.inc) at the bench's default shape: 256 streams x 16 blocks x 262144
bytes = 1 GiB of IQ resident on the device, Hann window, N = 1024, then N = 256 and 4096.

HIP events (torch.cuda.Event) on the launch stream around every launch; warm-up launches, then the median of --reps launches.  Printed per N:
ms, bytes/s of IQ read and the share of 8 TB/s, the way bench.py states its roofline; and, from the same session, the time of a
device-to-device hipMemcpyAsync of the same 1 GiB (which reads AND writes the bytes: 2 GiB of traffic) - the figure the kernel's read is
compared with.  One JSON line per measurement; --out also writes them to a file.  The tool ends itself after --timeout seconds; run it on an idle device,
and under a timeout of the caller's too:

    timeout -k 10 300 python3 tools/spectrum_time.py --out profiles/<name>.json"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--block-len", type=int, default=262144)
    ap.add_argument("--bins", default="1024,256,4096")
    ap.add_argument("--reps", type=int, default=30, help="timed launches per measurement (>= 20)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=240, help="seconds after which the tool ends itself (SIGALRM), whatever it is waiting for")
    args = ap.parse_args()
    import signal
    signal.alarm(args.timeout)
    if args.reps < 20:
        ap.error("--reps must be at least 20")

    import torch
    import rtl_fm_player_amd as R
    dev = torch.device("cuda:0")
    S, B, BL = args.streams, args.blocks, args.block_len
    n_bytes = S * B * BL
    g = torch.Generator(device=dev).manual_seed(1)
    iq = torch.randint(0, 256, (n_bytes,), dtype=torch.uint8, device=dev, generator=g)
    b = R.BatchDemod(R.wbfm_config(block_len=BL, rate_in=300000, rate_out2=48000, mode=2), S, device=0)
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

    copy_dst = torch.empty_like(iq)
    torch.cuda.synchronize()
    t = timed(lambda: copy_dst.copy_(iq, non_blocking=True))
    emit(dict(what="d2d_copy", bytes=n_bytes, traffic_bytes=2 * n_bytes, bytes_per_s=n_bytes / (t["median_ms"] * 1e-3),
              traffic_share_of_8TBps=2 * n_bytes / (t["median_ms"] * 1e-3) / HBM_PEAK, **t))
    del copy_dst
    for n_bins in [int(x) for x in args.bins.split(",")]:
        power = torch.zeros((S, B, n_bins), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        t = timed(lambda: b.spectrum_device(iq, B, n_bins, power, window=R.WINDOW_HANN, hip_stream=st.cuda_stream))
        bps = n_bytes / (t["median_ms"] * 1e-3)
        emit(dict(what="spectrum", n_bins=n_bins, window="hann", streams=S, blocks=B, block_len=BL, bytes=n_bytes, bytes_per_s=bps,
                  share_of_8TBps=bps / HBM_PEAK, complex_samples_per_s=bps / 2, **t))
        assert bool(torch.isfinite(power).all()) and float(power.max()) > 0
    b.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
