#!/usr/bin/env python3
"""Time of the channel tuner (fmd_tuner_run_device, csrc/tuner.inc) at two sizes: 16 sources -> 256 channels x 16 blocks x 262144 bytes (the bench's
default batch, every stream a station of one of 16 captures: 64 MiB in, 1 GiB out) and 1 source -> 10 channels (one dongle, ten stations), T = 64,
P = 2400 (1 kHz steps of 2.4 Msps).

HIP events (torch.cuda.Event) on the launch stream around every launch - the tuner kernel and the state kernel behind it; warm-up launches, then
the median of --reps launches with p10 / p90.  Beside it, from the same session: a device-to-device copy of the same INPUT bytes, and the fused
kernel (FMD_MATH_FAST, 300 k stereo, offset_tuning) over the tuner's output bytes - the demodulator the tuner feeds.  One JSON line per
measurement; --out also writes them to a file.  The tool ends itself after --timeout seconds; run it on an idle device, and under a timeout of
the caller's too:

    timeout -k 10 300 python3 tools/tuner_time.py --out profiles/<name>.json"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_LANES = 256 * 4 * 16          # CUs x SIMDs x lanes of an MI355X: fused multiply-adds per clock
CLOCK = 2.4e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16:256,1:10", help="comma-separated sources:channels pairs")
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--block-len", type=int, default=262144)
    ap.add_argument("--rate", type=int, default=2400000)
    ap.add_argument("--step", type=int, default=1000)
    ap.add_argument("--bw", type=int, default=100000)
    ap.add_argument("--taps", type=int, default=64)
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
    dev = torch.device("cuda:0")
    B, bl, T = args.blocks, args.block_len, args.taps
    P = args.rate // args.step
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

    for size in args.sizes.split(","):
        S, K = (int(x) for x in size.split(":"))
        g = torch.Generator(device=dev).manual_seed(1)
        iq = torch.randint(0, 256, (S * B * bl,), dtype=torch.uint8, device=dev, generator=g)
        out = torch.zeros((K, B, bl), dtype=torch.uint8, device=dev)
        copy_dst = torch.empty_like(iq)
        torch.cuda.synchronize()
        t = timed(lambda: copy_dst.copy_(iq, non_blocking=True))
        copy_ms = t["median_ms"]
        emit(dict(what="d2d_copy_of_the_input", sources=S, bytes=iq.numel(), bytes_per_s=iq.numel() / (copy_ms * 1e-3), **t))
        del copy_dst

        tun = R.Tuner(R.FmdTunerConfig(args.rate, args.step, args.bw, T, bl, 0), S, K, device=0)
        for c in range(K):
            tun.set_channel(c, c % S, ((37 * c + 11) % (2 * P - 1)) - (P - 1), 1.0)
        torch.cuda.synchronize()
        t = timed(lambda: tun.run_device(iq, B, out, hip_stream=st.cuda_stream))
        tuner_ms = t["median_ms"]
        n_out = K * B * (bl // 2)
        fma = 2.0 * T * n_out
        emit(dict(what="tuner", sources=S, channels=K, blocks=B, block_len=bl, n_taps=T, period=P, in_bytes=iq.numel(), out_bytes=out.numel(),
                  out_samples_per_s=n_out / (tuner_ms * 1e-3), fir_fma=fma, fir_fma_share_of_valu_peak=fma / (tuner_ms * 1e-3) / (VALU_LANES * CLOCK),
                  ratio_to_copy_of_the_input=tuner_ms / copy_ms, **t))
        tun.sync()
        assert int(out.max()) > int(out.min())

        cfg = R.wbfm_config(rate_in=args.rate // 8, rate_out2=48000, mode=2, block_len=bl, math=R.MATH_FAST, offset_tuning=True)
        b = R.BatchDemod(cfg, K, device=0)
        b.set_timing(False)
        pcm = torch.zeros(K * B * b.pcm_stride, dtype=torch.int16, device=dev)
        lens = torch.zeros(K * B, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        t = timed(lambda: b.run_device(out, B, pcm, lens, hip_stream=st.cuda_stream))
        emit(dict(what="fused_kernel_on_the_tuner_output", streams=K, blocks=B, block_len=bl, kernel=b.kernel_name(),
                  tuner_ratio_to_fused=tuner_ms / t["median_ms"], **t))
        b.sync()
        b.close()
        tun.close()
        del iq, out, pcm, lens
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
