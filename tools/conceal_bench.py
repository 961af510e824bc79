#!/usr/bin/env python3
"""Side measurement: the concealment machine's tick ("Concealment
machine"), device form, under four loss conditions, and its no-loss tick
against the good-packet step it is built on.

    python tools/conceal_bench.py [--batches 1024,8192] [--ticks 40] [--rounds 5] [--out FILE]
                                  [--noncausal | --delay D]

Per batch, on a model with the predictor's default shape, device-resident
PCM (a resonated pulse train plus noise per stream, 16 frames cycled), after
a 100 ms preheat with the workload itself:

  loss0    no loss
  loss3    every stream loses every tick with probability 3 %, independently
  loss10   the same with probability 10 %
  burst10  10 % of the ticks lost, in bursts of 3
  first    the worst tick: every stream meets its first loss in the same tick
           (four received ticks, then the timed one; repeated from a reset)

Each condition: `ticks` ticks queued back to back and one synchronisation,
wall time per tick with the timers off; then the same ticks with the timers
on for lpcnet_batch_kernel_ms by region (0 sample kernel, 1 frame kernel,
2 predictor, 3 extractor, 6 Burg analysis; the glue kernels of
conceal_kernel.hip are in no region: wall minus the regions bounds them and
the host's planning together).

The yardstick: the no-loss tick against lpcnet_batch_plc_update_device on a
twin batch (the same Burg, extractor and predictor launches without the
machine's bookkeeping), `rounds` alternating runs of `ticks` calls each in
one process; median, minimum and maximum of each and the median difference.

--noncausal opens the machine in the non-causal mode, which needs
FEATURES_DELAY 0 and sets it; --delay D sets FEATURES_DELAY for the causal
mode (0: the causal reference beside a non-causal run).  Every received
non-causal tick holds one frame of teacher-forced synthesis, so the floor is
reported too: `impl160`, the timed regions of
lpcnet_batch_synthesize_impl(N = 160, preload = 160) on the twin batch.
`*_kernel_ms` is the sum of a condition's timed regions per tick.
One JSON line per batch."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import lpcnet_amd as L  # noqa: E402

NFRAMES = 16
REGIONS = {0: "sample", 1: "frame", 2: "predictor", 3: "extractor", 6: "burg"}


def signals(B):
    """[NFRAMES, B, 160] int16: 64 distinct streams tiled over the batch."""
    n = NFRAMES * 160
    out = np.zeros((64, n))
    for s in range(64):
        rng = np.random.RandomState(900 + s)
        x = np.zeros(n)
        x[::40 + s] = 6000.0
        y = np.zeros(n + 2)
        for i in range(n):
            y[i + 2] = x[i] + 1.2 * y[i + 1] - 0.72 * y[i]
        out[s] = y[2:] + rng.randint(-20, 21, n)
    pcm = np.clip(np.rint(out), -32768, 32767).astype(np.int16).reshape(64, NFRAMES, 160)
    return np.ascontiguousarray(pcm[np.arange(B) % 64].transpose(1, 0, 2))


def loss_script(kind, B, ticks, rng):
    """[ticks, B] uint8."""
    if kind == "loss0":
        return np.zeros((ticks, B), np.uint8)
    if kind == "loss3":
        return (rng.rand(ticks, B) < .03).astype(np.uint8)
    if kind == "loss10":
        return (rng.rand(ticks, B) < .1).astype(np.uint8)
    if kind == "burst10":
        start = rng.rand(ticks, B) < .1 / 3
        lost = start.copy()
        lost[1:] |= start[:-1]
        lost[2:] |= start[:-2]
        return lost.astype(np.uint8)
    raise KeyError(kind)


class Bench:
    def __init__(self, blob, B, options=L.CONCEAL_CAUSAL, delay=None):
        self.B = B
        self.b = L.LPCNetBatch(B, 0, blob)
        self.twin = L.LPCNetBatch(B, 0, blob)
        if delay is not None:
            self.b.set_model_constants(1.0, delay, False)
            self.twin.set_model_constants(1.0, delay, False)
        self.b.conceal_open(options)
        pcm = signals(B)
        self.frame_bytes = B * 320
        self.d_in = [self.b.device_alloc(pcm.nbytes), self.twin.device_alloc(pcm.nbytes)]
        self.b.h2d(self.d_in[0], pcm)
        self.twin.h2d(self.d_in[1], pcm)
        self.pcm = pcm
        self.d_out = self.twin.device_alloc(B * 20 * 4)

    def run(self, lost):
        """The ticks of `lost` queued back to back; wall ms per tick.  A
        received tick reads its frame in place from the cycled input (update
        leaves it unchanged without a blend; a blended frame is rewritten
        here and a lost tick writes its concealed frame there, which changes
        the signal of later cycles, not the work)."""
        b = self.b
        b.h2d(self.d_in[0], self.pcm)  # concealed frames of the previous run out of the input
        b.sync()
        t0 = time.perf_counter()
        for t, row in enumerate(lost):
            b.conceal_frame_device(self.d_in[0] + (t % NFRAMES) * self.frame_bytes, row)
        b.sync()
        return (time.perf_counter() - t0) * 1e3 / len(lost)

    def restart(self):
        """Every stream from a reset and past the silent first frames: a frame
        concealed from here on is a signal, fit to be read back as a received one."""
        self.b.conceal_reset()
        self.run(np.zeros((4, self.B), np.uint8))

    def baseline(self, ticks):
        tw = self.twin
        t0 = time.perf_counter()
        for t in range(ticks):
            tw.plc_update_device(self.d_in[1] + (t % NFRAMES) * self.frame_bytes, self.d_out)
        tw.sync()
        return (time.perf_counter() - t0) * 1e3 / ticks

    def impl160(self, ticks):
        """The timed regions of a full frame of teacher-forced synthesis on the twin, per call."""
        tw = self.twin
        feats = L.synthetic_features(5, 1)[:, :20].repeat(self.B, 0)
        pcm = np.ascontiguousarray(self.pcm[0])
        tw.synthesize_impl(feats, pcm, 160)
        tw.reset_timers(2)
        for t in range(ticks):
            tw.synthesize_impl(feats, self.pcm[t % NFRAMES], 160)
        out = {name: round(tw.kernel_ms(w)[0] / ticks, 5) for w, name in REGIONS.items() if w < 2}
        tw.reset_timers(0)
        tw.reset()
        return out

    def regions(self, lost):
        b = self.b
        b.reset_timers(2)
        self.run(lost)
        out = {}
        for w, name in REGIONS.items():
            ms, n = b.kernel_ms(w)
            out[name] = {"ms_per_tick": round(ms / len(lost), 5), "launches_per_tick": round(n / len(lost), 2)}
        b.reset_timers(0)
        return out

    def first_loss(self, reps):
        """Four received ticks from a reset, then every stream lost at once: that tick alone."""
        b = self.b
        walls = []
        reg = {name: [0.0, 0] for name in REGIONS.values()}
        for timed in (False, True):
            for _ in range(reps):
                self.restart()
                if timed:
                    b.reset_timers(2)
                w = self.run(np.ones((1, self.B), np.uint8))
                if not timed:
                    walls.append(w)
                    continue
                for k, name in REGIONS.items():
                    ms, n = b.kernel_ms(k)
                    reg[name][0] += ms
                    reg[name][1] += n
        reg = {name: {"ms_per_tick": round(ms / reps, 5), "launches_per_tick": round(n / reps, 2)} for name, (ms, n) in reg.items()}
        b.reset_timers(0)
        return walls, reg

    def close(self):
        self.b.close()
        self.twin.close()


def spread(v):
    return {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}


def kernel_ms(regions):
    return round(sum(v["ms_per_tick"] for v in regions.values()), 5)


def measure(blob, B, ticks, rounds, preheat_ms, options=L.CONCEAL_CAUSAL, delay=None):
    x = Bench(blob, B, options, delay)
    rng = np.random.RandomState(11)
    t_end = time.perf_counter() + preheat_ms * 1e-3
    while time.perf_counter() < t_end:
        x.run(loss_script("loss3", B, 8, rng))
        x.baseline(8)
    r = {"streams": B, "ticks": ticks, "rounds": rounds, "plc_dims": list(L.plc_dims(blob)), "tick_ms": 10.0,
         "mode": "noncausal" if options & 3 == L.CONCEAL_NONCAUSAL else "causal", "features_delay": x.b.info().features_delay}
    r["impl160_regions_ms"] = x.impl160(ticks)
    # the yardstick first, alternating, from a reset
    x.restart()
    x.twin.reset()
    base, mach = [], []
    for _ in range(rounds):
        base.append(x.baseline(ticks))
        mach.append(x.run(loss_script("loss0", B, ticks, rng)))
    r["plc_update_device_wall_ms"] = spread(base)
    r["loss0_wall_ms"] = spread(mach)
    r["loss0_minus_plc_update_ms"] = round(statistics.median(mach) - statistics.median(base), 5)
    r["loss0_regions"] = x.regions(loss_script("loss0", B, ticks, rng))
    r["loss0_kernel_ms"] = kernel_ms(r["loss0_regions"])
    for kind in ("loss3", "loss10", "burst10"):
        x.restart()
        lost = loss_script(kind, B, ticks, rng)
        r[kind + "_lost_fraction"] = round(float(lost.mean()), 4)
        r[kind + "_wall_ms"] = spread([x.run(lost) for _ in range(rounds)])
        r[kind + "_regions"] = x.regions(lost)
        r[kind + "_kernel_ms"] = kernel_ms(r[kind + "_regions"])
    walls, reg = x.first_loss(rounds)
    r["first_wall_ms"] = spread(walls)
    r["first_regions"] = reg
    x.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1024,8192")
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--preheat-ms", type=float, default=100.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--noncausal", action="store_true", help="the non-causal mode, at FEATURES_DELAY 0")
    ap.add_argument("--delay", type=int, default=None, help="FEATURES_DELAY of the causal run (default: the model's)")
    a = ap.parse_args()
    if a.noncausal and a.delay not in (None, 0):
        sys.exit("conceal_bench: the non-causal mode needs FEATURES_DELAY 0")
    options, delay = (L.CONCEAL_NONCAUSAL, 0) if a.noncausal else (L.CONCEAL_CAUSAL, a.delay)
    if L.device_count() < 1:
        sys.exit("conceal_bench: no HIP device visible")
    blob = L.synthetic_model(1, L.VARIANT_INT8, plc=True)
    lines = []
    for B in [int(v) for v in a.batches.split(",")]:
        r = measure(blob, B, a.ticks, a.rounds, a.preheat_ms, options, delay)
        print(json.dumps(r), flush=True)
        lines.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
