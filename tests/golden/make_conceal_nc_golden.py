#!/usr/bin/env python3
"""Generates tests/golden/conceal_noncausal.npz (run where oracle/_ref is built).

The fixture of the concealment machine's non-causal mode, computed by
tests/conceal_nc_ref.py (ConcealNcRef: lpcnet_plc.c:342-492 restated line by
line over the checkers of the synthesis, the analysis, the Burg analysis and
the predictor): two runs, without and with the DC filter, on the small
predictor shape at FEATURES_DELAY 0; six streams each, on the six scripts of
conceal_ref.SCRIPTS over the signals of conceal_ref.received_pcm().  Per run:
the PCM of every tick and, after the last one, the control fields,
queued_update, queued_samples, dc_buf, st->features, st->pcm[0 .. 160),
dc_mem / syn_dc, the synthesis GRU states and frame_count, the predictor's
state and the analysis state of every stream.

Every frame that reaches burg_cepstral_analysis is checked against Burg's
contract before it is used (with the DC filter: the first DC pass of the
received frame); a frame outside it stops the stream, and the maker then tries
the stream on the other signals of tests/feat_signals.py in their order and
records which one it took (r_signals, r_pcm_in).  A stream that no signal
carries stops the maker.

Usage: python3 tests/golden/make_conceal_nc_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import conceal_nc_ref as NR  # noqa: E402
import conceal_ref as CR  # noqa: E402
import enc_ref  # noqa: E402
import feat_signals as FS  # noqa: E402


def stream_of(options, s, taken):
    """Stream s of a run on its own signal or, where that leaves Burg's
    contract, on the first other one that stays inside: (name, pcm_in, arrays)."""
    own = CR.SIGNALS[s]
    for name in [own] + [n for n in FS.INT16 if n not in CR.SIGNALS and n not in taken]:
        pcm = NR.signal_pcm(name)
        try:
            out = NR.compute_run(options, {s: pcm}, streams=[s])
        except ValueError as e:
            print("    stream %d on %s: %s" % (s, name, e))
            continue
        return name, pcm, out
    raise SystemExit("stream %d: no signal stays inside Burg's contract" % s)


def main():
    assert enc_ref.have_ref(), "oracle/_ref/libref_kernels.so missing: run `make -C oracle` with the reference tree present"
    arrays = {"lost": CR.lost_matrix(), "fec_events": np.stack([CR.fec_events(s) for s in range(len(CR.SCRIPTS))])}
    for run, options in NR.RUNS:
        names, pcm_in, parts = [], [], []
        for s in range(len(CR.SCRIPTS)):
            name, pcm, out = stream_of(options, s, names)
            names.append(name)
            pcm_in.append(pcm)
            parts.append(out)
        arrays[f"{run}_signals"] = np.array(names)
        arrays[f"{run}_pcm_in"] = np.stack(pcm_in)
        for k in NR.KEYS:
            arrays[f"{run}_{k}"] = np.concatenate([p[k] for p in parts])
        lost = arrays["lost"].astype(bool)
        print("  %-12s signals %s; concealed PCM |max| %d" % (run, ",".join(names), np.abs(arrays[f"{run}_pcm"][lost].astype(np.int32)).max()))
    np.savez_compressed(NR.GOLDEN, **arrays)
    print("wrote %s: %d arrays, %d bytes" % (NR.GOLDEN, len(arrays), os.path.getsize(NR.GOLDEN)))


if __name__ == "__main__":
    main()
