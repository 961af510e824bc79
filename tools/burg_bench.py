#!/usr/bin/env python3
"""Side measurement: the Burg analysis kernel's time per call beside the
feature extractor's and the PLC predictor's at the same batch, and the
good-packet step that chains the three ("burg_kernel").

    python tools/burg_bench.py [--batches 1024,8192,32768] [--out FILE]

Per batch, on device-resident int16 PCM (tools/feat_bench.py's signals, four
frames in rotation, every stream active): a 100 ms preheat with the Burg
kernel itself and 50 timed calls (lpcnet_batch_kernel_ms which = 6); 50 timed
extractor calls (which = 3); on a batch with a PLC model 50 timed
lpcnet_batch_plc_update_device calls, with their wall time per call and the
three kernels' times (which = 6, 3, 2) from the same calls.  When oracle/_ref
is built, also the reference's burg_cepstral_analysis per frame on one host
core, for scale.  One JSON line per batch."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import lpcnet_amd as L  # noqa: E402
import feat_bench  # noqa: E402

CALLS = 50
NFR = feat_bench.NFR
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libref_kernels.so")


def host_reference_us(pcm: np.ndarray):
    """The compiled reference's burg_cepstral_analysis, microseconds per frame
    on this core; None where oracle/_ref is not built."""
    if not os.path.exists(REF_SO):
        return None
    l = C.CDLL(REF_SO)
    l.burg_cepstral_analysis.argtypes = [C.c_void_p, C.c_void_p]
    l.burg_cepstral_analysis.restype = None
    frames = np.ascontiguousarray(pcm[:, :64].reshape(-1, L.FRAME_SIZE).astype(np.float32))
    out = np.zeros(36, np.float32)
    for x in frames[:16]:
        l.burg_cepstral_analysis(out.ctypes.data, x.ctypes.data)
    t0 = time.perf_counter()
    for x in frames:
        l.burg_cepstral_analysis(out.ctypes.data, x.ctypes.data)
    return (time.perf_counter() - t0) / len(frames) * 1e6


def timed_calls(b, call, which):
    b.reset_timers(1)
    t0 = time.perf_counter()
    for c in range(CALLS):
        call(c)
    b.sync()
    wall = (time.perf_counter() - t0) / CALLS
    return wall * 1e3, {w: b.kernel_ms(w) for w in which}


def measure(blob, B: int, preheat_ms: float) -> dict:
    pcm = feat_bench.signals(B)
    r = {"streams": B}
    b = L.LPCNetBatch(B, 0)  # no model: neither analysis has weights
    d_pcm = b.device_alloc(pcm.nbytes)
    d_out = b.device_alloc(B * L.BURG_CEPSTRUM * 4)
    d_feat = b.device_alloc(B * L.NB_FEATURES * 4)
    b.h2d(d_pcm, pcm)
    frame = [d_pcm + f * B * L.FRAME_SIZE * 2 for f in range(NFR)]
    t_end = time.perf_counter() + preheat_ms * 1e-3
    k = 0
    while time.perf_counter() < t_end:
        b.burg_cepstrum_device(frame[k % NFR], d_out)
        b.sync()
        k += 1
    wall, t = timed_calls(b, lambda c: b.burg_cepstrum_device(frame[c % NFR], d_out), (6,))
    r.update({"burg_kernel_ms_per_call": round(t[6][0] / max(1, t[6][1]), 5), "burg_launches": t[6][1],
              "burg_wall_ms_per_call": round(wall, 5)})
    wall, t = timed_calls(b, lambda c: b.compute_features_device(frame[c % NFR], d_feat, L.NB_FEATURES), (3,))
    r["extractor_kernel_ms_per_call"] = round(t[3][0] / max(1, t[3][1]), 5)
    for p in (d_pcm, d_out, d_feat):
        b.device_free(p)
    b.close()
    # the good-packet step: Burg + extractor into the row, then the predictor
    b = L.LPCNetBatch(B, 0, blob)
    d_pcm = b.device_alloc(pcm.nbytes)
    d_feat = b.device_alloc(B * L.NB_FEATURES * 4)
    b.h2d(d_pcm, pcm)
    frame = [d_pcm + f * B * L.FRAME_SIZE * 2 for f in range(NFR)]
    for c in range(5):
        b.plc_update_device(frame[c % NFR], d_feat)
    b.sync()
    b.reset_timers(0)
    t0 = time.perf_counter()
    for c in range(CALLS):
        b.plc_update_device(frame[c % NFR], d_feat)
    b.sync()
    r["update_wall_ms_per_call_untimed"] = round((time.perf_counter() - t0) / CALLS * 1e3, 5)
    wall, t = timed_calls(b, lambda c: b.plc_update_device(frame[c % NFR], d_feat), (6, 3, 2))
    per = {w: t[w][0] / max(1, t[w][1]) for w in t}
    r.update({"update_wall_ms_per_call": round(wall, 5), "update_burg_ms": round(per[6], 5), "update_extractor_ms": round(per[3], 5),
              "update_predictor_ms": round(per[2], 5), "update_kernel_sum_ms": round(per[6] + per[3] + per[2], 5),
              "update_launches": [t[6][1], t[3][1], t[2][1]], "tick_ms": 10.0,
              "burg_share_of_tick": round(r["burg_kernel_ms_per_call"] / 10.0, 5)})
    for p in (d_pcm, d_feat):
        b.device_free(p)
    b.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1024,8192,32768")
    ap.add_argument("--preheat-ms", type=float, default=100.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if L.device_count() < 1:
        sys.exit("burg_bench: no HIP device visible")
    blob = L.synthetic_model(1, L.VARIANT_INT8, plc=True)
    ref_us = host_reference_us(feat_bench.signals(64))
    lines = []
    for B in [int(v) for v in a.batches.split(",")]:
        r = measure(blob, B, a.preheat_ms)
        if ref_us is not None:
            r["reference_host_us_per_frame_one_core"] = round(ref_us, 3)
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
