#!/usr/bin/env python3
"""Side measurement: the feature extractor's kernel time per call beside the
PLC predictor's and the synthesis sample kernel's time per frame at the same
batch ("Feature extractor").

    python tools/feat_bench.py [--batches 1024,8192,32768] [--out FILE]

Per batch: tools/plc_bench.py's measurement (100 ms preheat with the
synthesis workload, 16 timed frames with which = 0, 50 timed predictor calls
with which = 2), then on a batch without a model a 100 ms preheat with the
extractor itself and 50 timed single-frame calls on device-resident PCM
(lpcnet_batch_kernel_ms which = 3), every stream active, four frames of
voiced, noisy and silent signals in rotation.  One JSON line per batch, with
the capacity tick's sum extractor + predictor + synthesis against 10 ms."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import lpcnet_amd as L  # noqa: E402
import plc_bench  # noqa: E402

CALLS = 50
NFR = 4


def signals(B: int) -> np.ndarray:
    """[NFR, B, 160] int16: 64 distinct streams (pulse trains of periods
    40..103 over noise, every eighth silent), cycled over the batch."""
    rng = np.random.RandomState(9)
    n = NFR * L.FRAME_SIZE
    base = np.zeros((64, n), np.float64)
    for s in range(64):
        if s % 8 == 7:
            continue
        base[s] = rng.randint(-300 * (1 + s % 5), 300 * (1 + s % 5) + 1, n)
        base[s, ::40 + s] += 9000
        for k in range(2, n):
            base[s, k] += 1.2 * base[s, k - 1] - 0.72 * base[s, k - 2]
    pcm = np.clip(np.rint(base), -32768, 32767).astype(np.int16).reshape(64, NFR, L.FRAME_SIZE)
    return np.ascontiguousarray(np.moveaxis(pcm, 0, 1)[:, np.arange(B) % 64])


def measure(B: int, preheat_ms: float) -> dict:
    pcm = signals(B)
    b = L.LPCNetBatch(B, 0)  # no model: the analysis has no weights
    d_pcm = b.device_alloc(pcm.nbytes)
    d_feat = b.device_alloc(B * L.NB_FEATURES * 4)
    b.h2d(d_pcm, pcm)
    frame = [d_pcm + f * B * L.FRAME_SIZE * 2 for f in range(NFR)]
    t_end = time.perf_counter() + preheat_ms * 1e-3
    k = 0
    while time.perf_counter() < t_end:
        b.compute_features_device(frame[k % NFR], d_feat, L.NB_FEATURES)
        b.sync()
        k += 1
    b.reset_timers(1)
    t0 = time.perf_counter()
    for c in range(CALLS):
        b.compute_features_device(frame[c % NFR], d_feat, L.NB_FEATURES)
    b.sync()
    wall = (time.perf_counter() - t0) / CALLS
    ms, n = b.kernel_ms(3)
    b.device_free(d_pcm)
    b.device_free(d_feat)
    b.close()
    return {"extractor_kernel_ms_per_call": round(ms / max(1, n), 5), "extractor_launches": n,
            "extractor_wall_ms_per_call": round(wall * 1e3, 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1024,8192,32768")
    ap.add_argument("--preheat-ms", type=float, default=100.0)
    ap.add_argument("--extractor-only", action="store_true", help="skip the synthesis and predictor measurement")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if L.device_count() < 1:
        sys.exit("feat_bench: no HIP device visible")
    blob = L.synthetic_model(1, L.VARIANT_INT8, plc=True)
    lines = []
    for B in [int(v) for v in a.batches.split(",")]:
        r = {"streams": B}
        if not a.extractor_only:
            p = plc_bench.measure(blob, B, a.preheat_ms)
            r.update({k: p[k] for k in ("predictor_kernel_ms_per_call", "synthesis_kernel_ms_per_frame", "synthesis_kernel")})
        r.update(measure(B, a.preheat_ms))
        if not a.extractor_only:
            r["extractor_over_synthesis"] = round(r["extractor_kernel_ms_per_call"] / r["synthesis_kernel_ms_per_frame"], 5)
            r["tick_ms"] = 10.0
            r["extractor_plus_predictor_plus_synthesis_ms"] = round(
                r["extractor_kernel_ms_per_call"] + r["predictor_kernel_ms_per_call"] + r["synthesis_kernel_ms_per_frame"], 5)
        if os.environ.get("LPCNET_LIB_VARIANT"):
            r["lib_variant"] = os.environ["LPCNET_LIB_VARIANT"]
        print(json.dumps(r), flush=True)
        lines.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
