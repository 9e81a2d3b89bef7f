#!/usr/bin/env python3
"""Time of stereo control (fmd_stereo_run_device, csrc/stereo.inc: pilot meter, tracker, apply) behind the fused kernel at the bench's shape: 256
streams x 16 blocks x 262144 bytes of IQ on the device (one block of the oracle's DDS multiplex, tiled), the PCM the FMD_MATH_FAST stereo batch
wrote for it, a z of 1024 complex values per block (what Batch.subcarrier(19000, 500) delivers there; its values do not bear on the time and
are random), the levels as quality, meters on, in place.

HIP events (torch.cuda.Event) on the launch stream around every launch; warm-up launches, then the median of --reps launches with p10 / p90.  From
the same session: the fused kernel's launch that produced the PCM, a device-to-device copy of the same PCM bytes (what any rewrite of the PCM has
to move at the least), the stereo launch in FMD_STEREO_AUTO (three kernels) and in FMD_STEREO_FORCE_STEREO without d_z (tracker and apply
alone: the difference is the pilot meter).  One JSON line per measurement; --out also writes them to a file.  The tool ends itself after --timeout
seconds; run it on an idle device, and under a timeout of the caller's too:

    timeout -k 10 300 python3 tools/stereo_time.py --out profiles/<name>.json"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--block-len", type=int, default=262144)
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
    from oracle import dds_bytes
    dev = torch.device("cuda:0")
    S, B, BL = args.streams, args.blocks, args.block_len
    iq = torch.from_numpy(dds_bytes(BL, stereo=1)).to(dev).repeat(S * B).contiguous()
    b = R.BatchDemod(R.wbfm_config(block_len=BL, rate_in=300000, rate_out2=48000, mode=2, math=R.MATH_FAST), S, device=0)
    stride, mz = b.pcm_stride, BL // 16 // 16
    pcm = torch.zeros(S * B * stride, dtype=torch.int16, device=dev)
    lens = torch.zeros(S * B, dtype=torch.int32, device=dev)
    levels = torch.zeros(S * B, dtype=torch.float32, device=dev)
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

    shape = dict(streams=S, blocks=B, block_len=BL, pcm_stride=stride, pilot_per_block=mz, pcm_bytes=pcm.numel() * 2)
    torch.cuda.synchronize()
    b.run_device_levels(iq, B, pcm, lens, levels, hip_stream=st.cuda_stream)          # the levels, once
    st.synchronize()
    b.reset()
    t = timed(lambda: b.run_device(iq, B, pcm, lens, hip_stream=st.cuda_stream))
    fused_ms = t["median_ms"]
    emit(dict(what="fused_kernel_launch", kernel=b.kernel_name(), iq_bytes=iq.numel(), **shape, **t))
    dst = torch.empty_like(pcm)
    t = timed(lambda: dst.copy_(pcm, non_blocking=True))
    copy_ms = t["median_ms"]
    emit(dict(what="d2d_copy_of_the_pcm", bytes_per_s=pcm.numel() * 2 / (copy_ms * 1e-3), **shape, **t))
    del dst
    keep = pcm.clone()                                      # the launches below rewrite the PCM in place, time after time: the values do not bear on the time
    z = (torch.rand((S * B * mz * 2,), dtype=torch.float32, device=dev) - 0.5) * 0.3
    info = torch.zeros(S * B * 32, dtype=torch.uint8, device=dev)
    meter = torch.zeros(S * B * 32, dtype=torch.uint8, device=dev)
    stc = R.Stereo(R.FmdStereoConfig(stride, mz, 2, 0, 0.05, 0.025, 0.05, 0.25, 0.25), S, device=0)
    torch.cuda.synchronize()
    for what, mode, d_z in (("stereo_auto_three_kernels", R.STEREO_AUTO, z), ("stereo_forced_tracker_and_apply", R.STEREO_FORCE_STEREO, None)):
        stc.reset()
        stc.set_mode(mode)
        pcm.copy_(keep)
        torch.cuda.synchronize()
        t = timed(lambda: stc.run_device(pcm, lens, d_z, levels, B, pcm, info, meter, hip_stream=st.cuda_stream))
        stc.sync()
        rec = info.cpu().numpy().view(R.STEREO_INFO_DTYPE)
        emit(dict(what=what, ratio_to_copy_of_the_pcm=t["median_ms"] / copy_ms, ratio_to_fused_kernel=t["median_ms"] / fused_ms,
                  pcm_bytes_per_s=2 * pcm.numel() * 2 / (t["median_ms"] * 1e-3), g_end_of_the_last_block=float(rec["g_end"][-1]),
                  frames_of_a_block=int(rec["frames"][0]), **shape, **t))
    stc.close()
    b.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
