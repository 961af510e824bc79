#!/usr/bin/env python3
"""Side measurement: the PLC predictor's kernel time per call beside the
synthesis sample kernel's time per frame at the same batch ("PLC
prediction network").

    python tools/plc_bench.py [--batches 1024,8192,32768] [--out FILE]

Per batch: a 100 ms preheat with the synthesis workload (bench.py's), then
16 timed frames (lpcnet_batch_kernel_ms which = 0 over the frames covered),
then 50 timed predictor calls on device-resident inputs (which = 2), every
stream active, a mix of the three input forms.  One JSON line per batch."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import lpcnet_amd as L  # noqa: E402

FRAMES = 16
CALLS = 50


def measure(blob, B, preheat_ms):
    feats = np.ascontiguousarray(
        np.stack([L.synthetic_features(s % 64, FRAMES)[:, :20] for s in range(64)], 1)[:, np.arange(B) % 64])
    b = L.LPCNetBatch(B, 0, blob)
    d_feat = b.device_alloc(feats.nbytes)
    d_pcm = b.device_alloc(FRAMES * B * 160 * 2)
    b.h2d(d_feat, feats)
    t_end = time.perf_counter() + preheat_ms * 1e-3
    while time.perf_counter() < t_end:
        b.synthesize_frames(None, d_feat, d_pcm, FRAMES)
        b.sync()
    b.reset()
    b.synthesize_frames(None, d_feat, d_pcm, 4)  # past the FEATURES_DELAY silence
    b.sync()
    b.reset_timers(1)
    b.synthesize_frames(None, d_feat, d_pcm, FRAMES)
    b.sync()
    ms, _ = b.kernel_ms(0)
    synth = ms / max(1, b.kernel_frames(0))
    # predictor: inputs of the three forms, one third of the streams each
    rng = np.random.RandomState(7)
    x = np.zeros((B, 57), np.float32)
    x[:, 36:56] = feats[0]
    x[:, 56] = np.where(np.arange(B) % 3 == 1, -1, 1)
    x[np.arange(B) % 3 == 2, :36] = (0.5 * rng.randn(int(np.sum(np.arange(B) % 3 == 2)), 36)).astype(np.float32)
    x[np.arange(B) % 3 == 0] = 0
    d_in = b.device_alloc(x.nbytes)
    d_out = b.device_alloc(B * 20 * 4)
    b.h2d(d_in, x)
    for _ in range(5):
        b.plc_predict_device(d_in, d_out)
    b.sync()
    b.reset_timers(1)
    t0 = time.perf_counter()
    for _ in range(CALLS):
        b.plc_predict_device(d_in, d_out)
    b.sync()
    wall = (time.perf_counter() - t0) / CALLS
    ms, n = b.kernel_ms(2)
    info = b.info()
    for p in (d_feat, d_pcm, d_in, d_out):
        b.device_free(p)
    b.close()
    pred = ms / max(1, n)
    return {"streams": B, "plc_dims": list(L.plc_dims(blob)), "predictor_kernel_ms_per_call": round(pred, 5),
            "predictor_launches": n, "predictor_wall_ms_per_call": round(wall * 1e3, 5),
            "synthesis_kernel_ms_per_frame": round(synth, 5), "synthesis_kernel": info.kernel_name,
            "predictor_over_synthesis": round(pred / synth, 5), "tick_ms": 10.0,
            "predictor_plus_synthesis_ms": round(pred + synth, 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1024,8192,32768")
    ap.add_argument("--preheat-ms", type=float, default=100.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if L.device_count() < 1:
        sys.exit("plc_bench: no HIP device visible")
    blob = L.synthetic_model(1, L.VARIANT_INT8, plc=True)
    lines = []
    for B in [int(v) for v in a.batches.split(",")]:
        r = measure(blob, B, a.preheat_ms)
        print(json.dumps(r), flush=True)
        lines.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
