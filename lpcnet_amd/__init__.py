"""lpcnet_amd -- Python mirror of the MI355X LPCNet synthesis engine.

Thin ctypes binding over ``liblpcnet_mi355x.so`` (built in-tree by
``make lib``).  The class API mirrors the reference C interface of
``include/lpcnet.h`` (auliaadila/LPCNet):

* :class:`LPCNet` -- one stream: ``lpcnet_create`` / ``lpcnet_load_model`` /
  ``lpcnet_synthesize`` / ``lpcnet_reset`` / ``lpcnet_destroy``
  (reference ``src/lpcnet.c:174-281``).
* :class:`LPCNetBatch` -- B independent streams on one GPU (the batch extension
  of ``include/lpcnet_mi355x.h``).

There is no CPU fallback: every synthesis call runs the HIP kernels, and
importing the package raises if the native library is absent.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# LPCNET_LIB_VARIANT=<name> loads liblpcnet_mi355x_<name>.so from this
# directory instead (in-tree A/B builds; still the native library, never a fallback)
LIB_PATH = os.path.join(_HERE, "liblpcnet_mi355x%s.so" % (
    "_" + os.environ["LPCNET_LIB_VARIANT"] if os.environ.get("LPCNET_LIB_VARIANT") else ""))

NB_FEATURES = 20
NB_TOTAL_FEATURES = 36
PLC_INPUTS = 57  # 2 NB_BANDS Burg cepstrum + NB_FEATURES + the loss flag (lpcnet_plc.c:149)
FRAME_SIZE = 160
BURG_CEPSTRUM = 36  # burg_cepstral_analysis: 18 half-sums and 18 differences of the half-frames' cepstra
PLC_ROW_BURG = 1    # LPCNET_PLC_ROW_BURG
PLC_ROW_FEATURES = 2  # LPCNET_PLC_ROW_FEATURES
VARIANT_INT8 = 0
VARIANT_FP32 = 1
CONCEAL_CAUSAL = 0     # LPCNET_CONCEAL_*: the reference's LPCNET_PLC_* values
CONCEAL_NONCAUSAL = 1  # FEATURES_DELAY 0 only
CONCEAL_CODEC = 2
CONCEAL_DC_FILTER = 4
CONCEAL_CTRL = ("pcm_fill", "skip_analysis", "blend", "loss_count", "fec_fill_pos", "fec_read_pos", "fec_keep_pos",
                "fec_skip", "feature_buffer_fill")


class LPCNetError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `make lib` (or __graft_entry__.build()); "
            "lpcnet_amd has no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    vp, i, f, u = C.c_void_p, C.c_int, C.c_float, C.c_uint
    sig = {
        "lpcnet_get_size": (i, []),
        "lpcnet_init": (i, [vp]),
        "lpcnet_create": (vp, []),
        "lpcnet_destroy": (None, [vp]),
        "lpcnet_reset": (None, [vp]),
        "lpcnet_synthesize": (None, [vp, vp, vp, i]),
        "lpcnet_load_model": (i, [vp, C.c_char_p, i]),
        "lpcnet_batch_create": (vp, [i, i]),
        "lpcnet_batch_destroy": (None, [vp]),
        "lpcnet_batch_load_model": (i, [vp, C.c_char_p, i]),
        "lpcnet_batch_model_info": (i, [vp, vp]),
        "lpcnet_batch_set_kernel": (i, [vp, i]),
        "lpcnet_batch_set_model_constants": (i, [vp, f, i, i]),
        "lpcnet_batch_set_rcp_table": (i, [vp, vp]),
        "lpcnet_mi355x_host_rcp_table": (i, [vp, i]),
        "lpcnet_mi355x_pool_stats": (i, [vp, vp, vp, vp]),
        "lpcnet_mi355x_set_placement": (i, [vp, i]),
        "lpcnet_mi355x_handle_placement": (i, [vp, vp, vp]),
        "lpcnet_batch_reset": (None, [vp]),
        "lpcnet_batch_reset_stream": (i, [vp, i]),
        "lpcnet_batch_nb_streams": (i, [vp]),
        "lpcnet_batch_synthesize": (i, [vp, vp, vp, i]),
        "lpcnet_batch_host_features": (C.POINTER(C.c_float), [vp]),
        "lpcnet_batch_host_pcm": (C.POINTER(C.c_short), [vp]),
        "lpcnet_batch_synthesize_impl": (i, [vp, vp, vp, i, i]),
        "lpcnet_batch_state_size": (i, []),
        "lpcnet_batch_save_state": (i, [vp, i, vp]),
        "lpcnet_batch_restore_state": (i, [vp, i, vp]),
        "lpcnet_batch_synthesize_frames": (i, [vp, vp, vp, vp, i, i]),
        "lpcnet_batch_sync": (i, [vp]),
        "lpcnet_batch_set_spin_limit": (i, [vp, i]),
        "lpcnet_batch_set_frame_chunking": (i, [vp, i]),
        "lpcnet_mi355x_validate_model": (i, [C.c_char_p, i]),
        "lpcnet_batch_device_alloc": (vp, [vp, C.c_size_t]),
        "lpcnet_batch_device_free": (i, [vp, vp]),
        "lpcnet_batch_memcpy_h2d": (i, [vp, vp, vp, C.c_size_t]),
        "lpcnet_batch_memcpy_d2h": (i, [vp, vp, vp, C.c_size_t]),
        "lpcnet_batch_reset_timers": (None, [vp, i]),
        "lpcnet_batch_kernel_ms": (C.c_double, [vp, i, C.POINTER(C.c_int)]),
        "lpcnet_batch_kernel_frames": (i, [vp, i]),
        "lpcnet_batch_set_stamps": (i, [vp, i]),
        "lpcnet_batch_get_stamps": (i, [vp, vp]),
        "lpcnet_batch_get_frame_stamps": (i, [vp, vp]),
        "lpcnet_batch_set_trace": (i, [vp, i]),
        "lpcnet_batch_get_trace": (i, [vp, vp, vp]),
        "lpcnet_batch_get_state": (i, [vp, i, vp, vp, vp, vp, vp, vp]),
        "lpcnet_mi355x_synthetic_model": (i, [u, i, i, vp, i]),
        "lpcnet_mi355x_synthetic_features": (None, [u, i, vp]),
        "lpcnet_mi355x_device_lpc": (i, [i, vp, vp, i]),
        "lpcnet_mi355x_rcp_table": (C.POINTER(C.c_uint32), []),
        "lpcnet_mi355x_device_count": (i, []),
        "lpcnet_mi355x_device_numerics": (i, [i, i, vp, vp, i]),
        "lpcnet_mi355x_last_error": (C.c_char_p, []),
        # reference-internal entry points on a handle (lpcnet_private.h:126-132)
        "lpcnet_synthesize_impl": (None, [vp, vp, vp, i, i]),
        "lpcnet_synthesize_tail_impl": (None, [vp, vp, i, i]),
        "run_frame_network_deferred": (None, [vp, vp]),
        "run_frame_network_flush": (None, [vp]),
        "lpcnet_reset_signal": (None, [vp]),
        "lpcnet_mi355x_state_size": (i, []),
        "lpcnet_mi355x_state_save": (i, [vp, vp]),
        "lpcnet_mi355x_state_restore": (i, [vp, vp]),
        "lpcnet_mi355x_deinit": (None, [vp]),
        # 1.6 kb/s decoder (include/lpcnet.h:63-100)
        "lpcnet_decoder_get_size": (i, []),
        "lpcnet_decoder_init": (i, [vp]),
        "lpcnet_decoder_create": (vp, []),
        "lpcnet_decoder_destroy": (None, [vp]),
        "lpcnet_decode": (i, [vp, vp, vp]),
        "lpcnet_mi355x_decoder_load_model": (i, [vp, C.c_char_p, i]),
        "lpcnet_batch_synthesize_tail_impl": (i, [vp, vp, i, i]),
        "lpcnet_batch_run_frame_network": (i, [vp, vp, i]),
        "lpcnet_batch_reset_signal": (i, [vp, i]),
        "lpcnet_batch_decode": (i, [vp, vp, vp]),
        "lpcnet_batch_decode_frames": (i, [vp, vp, vp, i]),
        # PLC prediction network (compute_plc_pred, lpcnet_plc.c:135-145)
        "lpcnet_mi355x_plc_dims": (i, [C.c_char_p, i, vp]),
        "lpcnet_mi355x_side_digest": (i, [C.c_char_p, i, vp, i]),
        "lpcnet_batch_plc_info": (i, [vp, vp]),
        "lpcnet_batch_plc_predict": (i, [vp, vp, vp, vp]),
        "lpcnet_batch_plc_predict_device": (i, [vp, vp, vp, vp]),
        "lpcnet_batch_plc_reset": (i, [vp, i]),
        "lpcnet_batch_plc_state_size": (i, [vp]),
        "lpcnet_batch_plc_save_state": (i, [vp, i, vp]),
        "lpcnet_batch_plc_restore_state": (i, [vp, i, vp]),
        # DRED RDO-VAE (dred_rdovae_enc.c, dred_rdovae_dec.c, dred_rdovae.c)
        "lpcnet_mi355x_rdovae_dims": (i, [C.c_char_p, i, vp]),
        "lpcnet_batch_rdovae_info": (i, [vp, vp]),
        "lpcnet_batch_rdovae_encode": (i, [vp, vp, vp, vp, vp]),
        "lpcnet_batch_rdovae_encode_device": (i, [vp, vp, i, vp, vp, vp]),
        "lpcnet_batch_rdovae_dec_init": (i, [vp, vp, vp]),
        "lpcnet_batch_rdovae_dec_init_device": (i, [vp, vp, vp]),
        "lpcnet_batch_rdovae_decode_qframe": (i, [vp, vp, vp, vp]),
        "lpcnet_batch_rdovae_decode_qframe_device": (i, [vp, vp, vp, vp]),
        "lpcnet_batch_rdovae_decode_all": (i, [vp, vp, vp, vp, i, vp]),
        "lpcnet_batch_rdovae_decode_all_device": (i, [vp, vp, vp, vp, i, vp]),
        "lpcnet_batch_rdovae_reset": (i, [vp, i, i]),
        "lpcnet_batch_rdovae_state_size": (i, [vp, i]),
        "lpcnet_batch_rdovae_save_state": (i, [vp, i, i, vp]),
        "lpcnet_batch_rdovae_restore_state": (i, [vp, i, i, vp]),
        # feature extraction (lpcnet_compute_single_frame_features)
        "lpcnet_batch_compute_features": (i, [vp, vp, vp, vp]),
        "lpcnet_batch_compute_features_float": (i, [vp, vp, vp, vp]),
        "lpcnet_batch_compute_features_device": (i, [vp, vp, vp, i, vp, i]),
        "lpcnet_batch_features_reset": (i, [vp, i]),
        "lpcnet_batch_features_state_size": (i, [vp]),
        "lpcnet_batch_features_save_state": (i, [vp, i, vp]),
        "lpcnet_batch_features_restore_state": (i, [vp, i, vp]),
        # Burg cepstral analysis and the predictor's input rows
        "lpcnet_batch_burg_cepstrum": (i, [vp, vp, vp, vp]),
        "lpcnet_batch_burg_cepstrum_float": (i, [vp, vp, vp, vp]),
        "lpcnet_batch_burg_cepstrum_device": (i, [vp, vp, vp, i, i, vp, i]),
        "lpcnet_batch_plc_rows_device": (i, [vp, vp, vp, i, f, vp]),
        "lpcnet_batch_plc_update": (i, [vp, vp, vp, vp]),
        "lpcnet_batch_plc_update_device": (i, [vp, vp, vp, vp]),
        # 1.6 kb/s encoder (lpcnet_encode, lpcnet_compute_features)
        "lpcnet_batch_encode": (i, [vp, vp, vp, vp, vp]),
        "lpcnet_batch_compute_features4": (i, [vp, vp, vp, vp]),
        "lpcnet_batch_encode_device": (i, [vp, vp, vp, vp, i, vp, i]),
        "lpcnet_batch_encode_state_size": (i, [vp]),
        "lpcnet_batch_encode_save_state": (i, [vp, i, vp]),
        "lpcnet_batch_encode_restore_state": (i, [vp, i, vp]),
        "lpcnet_mi355x_enc_main_pitch": (i, [vp, vp, i]),
        # concealment machine (lpcnet_plc_update / lpcnet_plc_conceal)
        "lpcnet_batch_conceal_open": (i, [vp, i]),
        "lpcnet_batch_conceal_close": (i, [vp]),
        "lpcnet_batch_conceal_reset": (i, [vp, i]),
        "lpcnet_batch_conceal_frame": (i, [vp, vp, vp, vp]),
        "lpcnet_batch_conceal_frame_device": (i, [vp, vp, vp, vp]),
        "lpcnet_batch_conceal_fec_add": (i, [vp, i, vp]),
        "lpcnet_batch_conceal_fec_clear": (i, [vp, i]),
        "lpcnet_batch_conceal_get_state": (i, [vp, i, vp, vp, vp, vp]),
        "lpcnet_batch_conceal_get_state_noncausal": (i, [vp, i, vp, vp, vp]),
        "lpcnet_mi355x_conceal_plan": (i, [i, i, vp, vp, i, vp, i, vp, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


class ModelInfo(C.Structure):
    _fields_ = [("variant", C.c_int), ("gru_a_blocks", C.c_int), ("gru_b_blocks", C.c_int),
                ("may_saturate", C.c_int), ("bytes_shared_per_frame", C.c_double),
                ("bytes_shared_per_sample", C.c_double), ("bytes_per_stream_sample", C.c_double),
                ("ops_per_sample", C.c_double), ("streams_per_workgroup", C.c_int), ("quad_path", C.c_int),
                ("lds_bytes", C.c_int), ("mfma_ops_per_group_sample", C.c_double),
                ("lpc_gamma", C.c_float), ("features_delay", C.c_int), ("end2end", C.c_int),
                ("long_rows", C.c_int), ("has_codebooks", C.c_int), ("rcp_hw", C.c_int)]

    @property
    def kernel_name(self) -> str:
        """Demangled template instance of the sample kernel this model runs
        (as rocprofv3 names it)."""
        sat = "true" if self.may_saturate else "false"
        lr = "true" if self.long_rows else "false"
        hw = "true" if self.rcp_hw else "false"
        if self.quad_path == 4:
            return f"mf_kernel<{self.streams_per_workgroup}, 0, {lr}, {hw}>"
        if self.quad_path == 6:
            return f"mf2_kernel<4, {lr}, {hw}>"
        if self.quad_path == 7:
            return f"mfw_kernel<true, {self.streams_per_workgroup // 4}, {lr}>"
        if self.quad_path == 5:
            return f"fp_kernel<0, {lr}, {hw}>"
        quad = "true" if self.quad_path == 1 else "false"
        return f"sample_kernel<{self.streams_per_workgroup}, {self.variant}, {sat}, {quad}>"


def last_error() -> str:
    return (lib.lpcnet_mi355x_last_error() or b"").decode()


def device_numerics(op: int, x: np.ndarray, n: int | None = None, device: int = 0) -> np.ndarray:
    """Run one device-numerics routine (see lpcnet_mi355x_device_numerics)
    on the GPU; x is reinterpreted as 32-bit words, the result is uint32."""
    src = np.ascontiguousarray(x).view(np.uint32)
    cnt = int(n if n is not None else src.size)
    out = np.zeros(cnt, np.uint32)
    if lib.lpcnet_mi355x_device_numerics(device, op, src.ctypes.data, out.ctypes.data, cnt) != 0:
        raise LPCNetError("device numerics failed: " + last_error())
    return out


def validate_model(blob: bytes) -> None:
    """Host-only check of a weight blob with lpcnet_load_model's rules; raises LPCNetError."""
    if lib.lpcnet_mi355x_validate_model(blob, len(blob)) != 0:
        raise LPCNetError(last_error())


def device_count() -> int:
    return lib.lpcnet_mi355x_device_count()


def set_placement(devices) -> None:
    """Placement list of drop-in handles initialised from now on (a device
    may appear twice); [] restores the default (every visible device)."""
    arr = (C.c_int * max(len(devices), 1))(*devices)
    if lib.lpcnet_mi355x_set_placement(arr, len(devices)) != 0:
        raise LPCNetError(last_error())


def synthetic_model(seed: int = 1, variant: int = VARIANT_INT8, saturating: bool = False, skewed: bool = False,
                    codebooks: bool = False, plc: bool = False, plc_small: bool = False,
                    rdovae: bool = False, rdovae_small: bool = False) -> bytes:
    """Deterministic synthetic default-size model in the reference blob format.
    skewed: GRU_A masks by a global per-gate threshold over skewed block
    energies (Sparsify, training_tf2/lpcnet.py:140-160): long block rows.
    codebooks: append the 1.6 kb/s decoder's ceps codebooks (other arrays unchanged).
    plc: append the PLC prediction network's records in the reference's default
    shape (cond 128, 256 / 256 units); plc_small: in a small unequal shape
    (cond 64, 128 / 64 units) instead (other arrays unchanged).
    rdovae: append the DRED RDO-VAE's encoder and decoder records in
    dump_rdovae.py's default shape (stack 256 wide, T 2048, 80 latents, state
    24); rdovae_small: in a small unequal shape (T 704, 40 latents, state 32)
    instead (other arrays unchanged)."""
    flags = ((1 if saturating else 0) | (2 if skewed else 0) | (4 if codebooks else 0) |
             (8 if plc or plc_small else 0) | (16 if plc_small else 0) |
             (32 if rdovae or rdovae_small else 0) | (64 if rdovae_small else 0))
    n = lib.lpcnet_mi355x_synthetic_model(seed, variant, flags, None, 0)
    buf = C.create_string_buffer(n)
    lib.lpcnet_mi355x_synthetic_model(seed, variant, flags, buf, n)
    return buf.raw


def plc_dims(blob: bytes) -> tuple[int, int, int, int]:
    """(57, cond, units1, units2) of a blob's PLC prediction network (host only);
    raises LPCNetError with the reason if the blob has no usable PLC records."""
    d = (C.c_int * 4)()
    if lib.lpcnet_mi355x_plc_dims(blob, len(blob), d) != 0:
        raise LPCNetError(last_error())
    return tuple(d)


def _rdovae_dims_dict(d) -> dict:
    """lpcnet_mi355x_rdovae_dims' 24 values as {"enc": {...} | None, "dec": {...} | None}."""
    d = [int(v) for v in d]
    enc = dict(L=d[0], S=d[1], T=d[2], kernel=d[3], widths=tuple(d[4:12]), gdense1=d[12]) if d[2] else None
    dec = dict(L=d[13], S=d[14], T=d[15], widths=tuple(d[16:24])) if d[15] else None
    return {"enc": enc, "dec": dec}


def rdovae_dims(blob: bytes) -> dict:
    """The dimensions of a blob's DRED RDO-VAE (host only): {"enc": dict(L, S,
    T, kernel, widths, gdense1) or None, "dec": dict(L, S, T, widths) or
    None}; a side without usable records is None.  Raises LPCNetError with
    both reasons when neither side is usable."""
    d = (C.c_int * 24)()
    if lib.lpcnet_mi355x_rdovae_dims(blob, len(blob), d) != 0:
        raise LPCNetError(last_error())
    return _rdovae_dims_dict(d)


def side_digest(blob: bytes | None) -> list[int]:
    """lpcnet_mi355x_side_digest: FNV-1a-64 of the ten PLC tables of a blob (0
    without usable PLC records, or for None), of the LPC and feature-extractor
    tables, then the four PLC dims (host only)."""
    out = (C.c_uint64 * 16)()
    if lib.lpcnet_mi355x_side_digest(blob, len(blob) if blob else 0, out, 16) != 16:
        raise LPCNetError(last_error())
    return list(out)


def with_model_constants(blob: bytes, lpc_gamma: float | None = None, features_delay: int | None = None,
                         end2end: bool | None = None) -> bytes:
    """``blob`` plus the side records LPC_GAMMA / FEATURES_DELAY / END2END
    (64-byte WeightHead records, nnet.h:54-61) that carry the constants
    dump_lpcnet.py writes into nnet_data.h; the reference's parser skips
    records it does not bind."""
    out = bytearray(blob)
    for name, val in (("LPC_GAMMA", None if lpc_gamma is None else np.float32(lpc_gamma).tobytes()),
                      ("FEATURES_DELAY", None if features_delay is None else np.int32(features_delay).tobytes()),
                      ("END2END", None if end2end is None else np.int32(1 if end2end else 0).tobytes())):
        if val is None:
            continue
        head = bytearray(64)
        head[0:4] = b"DNNw"
        head[8:12] = np.int32(0 if name == "LPC_GAMMA" else 1).tobytes()  # WEIGHT_TYPE_float / _int
        head[12:16] = np.int32(4).tobytes()
        head[16:20] = np.int32(64).tobytes()
        head[20:20 + len(name)] = name.encode()
        out += head + val + bytes(60)
    return bytes(out)


def enc_main_pitch(center_pitch: np.ndarray) -> np.ndarray:
    """main_pitch of the 1.6 kb/s encoder (lpcnet_enc.c:678-679) for every
    float32 center_pitch, from the kernel's threshold table (host only)."""
    x = np.ascontiguousarray(center_pitch, np.float32).ravel()
    out = np.zeros(x.size, np.int32)
    if lib.lpcnet_mi355x_enc_main_pitch(x.ctypes.data, out.ctypes.data, x.size) != 0:
        raise LPCNetError(last_error())
    return out


def conceal_plan(options: int, features_delay: int, lost, fec_adds=None):
    """The concealment machine's planner on one stream from reset (host only):
    lost [nticks] (non-zero: the tick's packet is lost); fec_adds [nticks] or
    None: before tick t, n > 0 FEC adds, -1 a NULL add, -2 a clear.  Returns
    (steps, ctrl): per tick the list of (op, a, b) primitive calls of
    lpcnet_plc.c in order (conceal_plan.h names them) and the control fields
    after the tick as a dict keyed by CONCEAL_CTRL."""
    lo = np.ascontiguousarray(np.asarray(lost) != 0, np.uint8)
    n = lo.size
    fa = None if fec_adds is None else np.ascontiguousarray(fec_adds, np.int32)
    if fa is not None and fa.shape != (n,):
        raise ValueError(f"fec_adds must be [{n}]")
    end = np.zeros(max(n, 1), np.int32)
    ctrl = np.zeros((max(n, 1), len(CONCEAL_CTRL)), np.int32)
    total = lib.lpcnet_mi355x_conceal_plan(options, features_delay, _ptr(lo), _ptr(fa), n, None, 0, None, None)
    if total < 0:
        raise LPCNetError(last_error())
    st = np.zeros((max(total, 1), 3), np.int32)
    if lib.lpcnet_mi355x_conceal_plan(options, features_delay, _ptr(lo), _ptr(fa), n, st.ctypes.data, total,
                                      end.ctypes.data, ctrl.ctypes.data) != total:
        raise LPCNetError(last_error())
    steps, first = [], 0
    for t in range(n):
        steps.append([tuple(int(v) for v in row) for row in st[first:end[t]]])
        first = int(end[t])
    return steps, [dict(zip(CONCEAL_CTRL, (int(v) for v in ctrl[t]))) for t in range(n)]


def synthetic_features(stream: int, nframes: int) -> np.ndarray:
    """[nframes, 36] float32 synthetic features of stream ``stream``."""
    out = np.zeros((nframes, NB_TOTAL_FEATURES), np.float32)
    lib.lpcnet_mi355x_synthetic_features(stream, nframes, out.ctypes.data)
    return out


def device_lpc(cepstra: np.ndarray, device: int = 0) -> np.ndarray:
    """lpc_from_cepstrum (freq.c:310-320) of cepstra [n, 18] on the GPU (lpc_kernel) -> [n, 16]."""
    c = np.ascontiguousarray(np.asarray(cepstra, np.float32).reshape(-1, 18))
    out = np.zeros((c.shape[0], 16), np.float32)
    if lib.lpcnet_mi355x_device_lpc(device, c.ctypes.data, out.ctypes.data, c.shape[0]) != 0:
        raise LPCNetError("device LPC failed: " + last_error())
    return out


def host_rcp_table() -> tuple[np.ndarray, int]:
    """This host CPU's rcpps as the 4096-entry (top 12 mantissa bits) table
    and the number of mantissas/exponents that form does not reproduce."""
    t = np.zeros(4096, np.uint32)
    bad = lib.lpcnet_mi355x_host_rcp_table(t.ctypes.data, 4096)
    return t, bad


def rcp_table() -> np.ndarray:
    p = lib.lpcnet_mi355x_rcp_table()
    return np.ctypeslib.as_array(p, shape=(2048,)).copy()


class LPCNet:
    """One synthesis stream (reference LPCNetState semantics)."""

    def __init__(self, blob: bytes | None = None):
        self._st = lib.lpcnet_create()
        if not self._st:
            raise LPCNetError("lpcnet_create failed")
        if blob is not None:
            self.load_model(blob)

    def load_model(self, blob: bytes) -> None:
        if lib.lpcnet_load_model(self._st, blob, len(blob)) != 0:
            raise LPCNetError(f"lpcnet_load_model failed: {last_error()}")

    def reset(self) -> None:
        lib.lpcnet_reset(self._st)

    def synthesize(self, features: np.ndarray, n: int = FRAME_SIZE) -> np.ndarray:
        f = np.ascontiguousarray(features[:NB_FEATURES], np.float32)
        out = np.zeros(n, np.int16)
        lib.lpcnet_synthesize(self._st, f.ctypes.data, out.ctypes.data, n)
        return out

    # -- reference-internal entry points (lpcnet_private.h:126-132, the PLC's calls) --
    def synthesize_impl(self, features: np.ndarray, pcm: np.ndarray, preload: int) -> np.ndarray:
        """lpcnet_synthesize_impl: pcm [N] int16, the first ``preload`` samples teacher-forced."""
        f = np.ascontiguousarray(np.asarray(features, np.float32)[:NB_FEATURES])
        out = np.ascontiguousarray(pcm, np.int16).copy()
        lib.lpcnet_synthesize_impl(self._st, f.ctypes.data, out.ctypes.data if out.size else None, out.size, preload)
        return out

    def synthesize_tail_impl(self, pcm: np.ndarray, preload: int = 0) -> np.ndarray:
        """lpcnet_synthesize_tail_impl: the sample network only, on the current conditioning."""
        out = np.ascontiguousarray(pcm, np.int16).copy()
        lib.lpcnet_synthesize_tail_impl(self._st, out.ctypes.data if out.size else None, out.size, preload)
        return out

    def frame_deferred(self, features: np.ndarray) -> None:
        """run_frame_network_deferred (lpcnet.c:122-132)."""
        f = np.ascontiguousarray(np.asarray(features, np.float32)[:NB_FEATURES])
        lib.run_frame_network_deferred(self._st, f.ctypes.data)

    def frame_flush(self) -> None:
        """run_frame_network_flush (lpcnet.c:134-144)."""
        lib.run_frame_network_flush(self._st)

    def reset_signal(self) -> None:
        """lpcnet_reset_signal (lpcnet.c:226-233)."""
        lib.lpcnet_reset_signal(self._st)

    def save(self) -> bytes:
        """The handle's whole synthesis state (replaces the PLC's LPCNetState struct copy)."""
        buf = C.create_string_buffer(lib.lpcnet_mi355x_state_size())
        if lib.lpcnet_mi355x_state_save(self._st, buf) != 0:
            raise LPCNetError(last_error())
        return buf.raw

    def restore(self, state: bytes) -> None:
        if lib.lpcnet_mi355x_state_restore(self._st, state) != 0:
            raise LPCNetError(last_error())

    def placement(self) -> tuple[int, int]:
        """(device, placement index; -1 when pinned by LPCNET_DEVICE)."""
        d, p = C.c_int(), C.c_int()
        if lib.lpcnet_mi355x_handle_placement(self._st, C.byref(d), C.byref(p)) != 0:
            raise LPCNetError(last_error())
        return d.value, p.value

    def close(self) -> None:
        if self._st:
            lib.lpcnet_destroy(self._st)
            self._st = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LPCNetDecoder:
    """The 1.6 kb/s decoder: lpcnet_decoder_create / lpcnet_decode (lpcnet.c:283-319)."""

    def __init__(self, blob: bytes):
        self._st = lib.lpcnet_decoder_create()
        if not self._st:
            raise LPCNetError("lpcnet_decoder_create failed")
        if lib.lpcnet_mi355x_decoder_load_model(self._st, blob, len(blob)) != 0:
            err = last_error()
            self.close()
            raise LPCNetError(f"decoder model: {err}")

    def decode(self, packet: bytes) -> np.ndarray:
        """One 8-byte packet -> 640 int16 samples."""
        if len(packet) != 8:
            raise ValueError("a packet is 8 bytes")
        buf = C.create_string_buffer(bytes(packet), 8)
        out = np.zeros(4 * FRAME_SIZE, np.int16)
        if lib.lpcnet_decode(self._st, buf, out.ctypes.data) != 0:
            raise LPCNetError(last_error())
        return out

    def close(self) -> None:
        if self._st:
            lib.lpcnet_decoder_destroy(self._st)
            self._st = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _BatchOwner:
    """Owns the native batch: lpcnet_batch_destroy runs when the last
    reference goes -- the LPCNetBatch (until close()) or an array handed out
    by host_features() / synthesize_host(), whose buffer object holds this
    owner, so such an array never outlives the host-visible memory it views."""

    def __init__(self, ptr):
        self.ptr = ptr

    def __del__(self):
        if self.ptr:
            lib.lpcnet_batch_destroy(self.ptr)
            self.ptr = None


def _pcm_arg(pcm, shape: tuple[int, int], float_ok: bool = False) -> np.ndarray:
    """The caller's PCM as a contiguous array of ``shape``: int16, or with
    float_ok float32 as well (the reference's short -> float conversion done)."""
    p = np.ascontiguousarray(pcm)
    if float_ok:
        if p.dtype not in (np.int16, np.float32):
            raise ValueError("pcm must be int16 or float32")
        if p.shape != shape:
            raise ValueError(f"pcm must be [{shape[0]}, {shape[1]}]")
    elif p.dtype != np.int16 or p.shape != shape:
        raise ValueError(f"pcm must be int16 [{shape[0]}, {shape[1]}]")
    return p


def _active_arg(active, B: int) -> np.ndarray | None:
    """The active mask as B bytes (None: every stream)."""
    a = None if active is None else np.ascontiguousarray(np.asarray(active) != 0, np.uint8)
    if a is not None and a.shape != (B,):
        raise ValueError(f"active must be [{B}]")
    return a


def _out_arg(out, shape: tuple, dtype=np.float32, what: str = "out") -> np.ndarray:
    """The caller's ``out``, used in place (rows of inactive streams keep their
    content), or zeros without one."""
    o = np.zeros(shape, dtype) if out is None else out
    if o.dtype != dtype or o.shape != shape or not o.flags.c_contiguous:
        raise ValueError(f"{what} must be a contiguous {np.dtype(dtype).name} [{', '.join(map(str, shape))}]")
    return o


def _ptr(a: np.ndarray | None):
    return None if a is None else a.ctypes.data


def _save_snapshot(save, b, stream: int, size: int) -> bytes:
    if size < 0:
        raise LPCNetError(last_error())
    buf = C.create_string_buffer(size)
    if save(b, stream, buf) != 0:
        raise LPCNetError(last_error())
    return buf.raw


def _restore_snapshot(restore, b, stream: int, state: bytes, size: int, wrong_size: str) -> None:
    if len(state) != size:
        raise LPCNetError(wrong_size)
    if restore(b, stream, state) != 0:
        raise LPCNetError(last_error())


def _owned_view(owner: _BatchOwner, addr: int, ctype, dtype, shape) -> np.ndarray:
    n = int(np.prod(shape))
    buf = (ctype * n).from_address(addr)
    buf._owner = owner  # the array's base keeps the native batch alive
    return np.frombuffer(buf, dtype=dtype).reshape(shape)


class LPCNetBatch:
    """B independent streams on one MI355X (include/lpcnet_mi355x.h)."""

    def __init__(self, nb_streams: int, device: int = 0, blob: bytes | None = None):
        self._b = lib.lpcnet_batch_create(nb_streams, device)
        if not self._b:
            raise LPCNetError(f"lpcnet_batch_create failed: {last_error()}")
        self._owner = _BatchOwner(self._b)
        self.B = nb_streams
        if blob is not None:
            self.load_model(blob)

    def load_model(self, blob: bytes) -> None:
        if lib.lpcnet_batch_load_model(self._b, blob, len(blob)) != 0:
            raise LPCNetError(f"lpcnet_batch_load_model failed: {last_error()}")

    def set_kernel(self, mode: int) -> None:
        """0 automatic, 1 lockstep sample kernel, 4 mf_kernel (matrix cores), 5 fp_kernel (fp32);
        a mode the model cannot run falls back to 1."""
        if lib.lpcnet_batch_set_kernel(self._b, mode) != 0:
            raise LPCNetError(last_error())

    def set_model_constants(self, lpc_gamma: float = 1.0, features_delay: int = 2, end2end: bool = False) -> None:
        """LPC_GAMMA / FEATURES_DELAY / END2END of the loaded model (the reference's
        nnet_data.h constants); see lpcnet_batch_set_model_constants."""
        if lib.lpcnet_batch_set_model_constants(self._b, lpc_gamma, features_delay, 1 if end2end else 0) != 0:
            raise LPCNetError(last_error())

    def set_rcp_table(self, table: np.ndarray | None) -> None:
        """Same-box parity: the rcpps table of the device activations (4096
        entries, see host_rcp_table; None = the default Intel table)."""
        t = None if table is None else np.ascontiguousarray(table, np.uint32)
        if t is not None and t.size != 4096:
            raise ValueError("rcpps table must have 4096 entries (top 12 mantissa bits, see host_rcp_table); "
                             f"got {t.size}")
        if lib.lpcnet_batch_set_rcp_table(self._b, None if t is None else t.ctypes.data) != 0:
            raise LPCNetError(last_error())

    def set_spin_limit(self, polls: int) -> None:
        """LDS flag-wait bound of the barrier-free kernel (0 = default); see lpcnet_mi355x.h."""
        if lib.lpcnet_batch_set_spin_limit(self._b, polls) != 0:
            raise LPCNetError("bad spin limit")

    def set_frame_chunking(self, enable: bool) -> None:
        """Chunked frame network for batches above 128 streams (default on); off = per-frame kernel."""
        if lib.lpcnet_batch_set_frame_chunking(self._b, 1 if enable else 0) != 0:
            raise LPCNetError("set_frame_chunking failed")

    def info(self) -> ModelInfo:
        mi = ModelInfo()
        if lib.lpcnet_batch_model_info(self._b, C.byref(mi)) != 0:
            raise LPCNetError("no model loaded")
        return mi

    def reset(self, stream: int | None = None) -> None:
        if stream is None:
            lib.lpcnet_batch_reset(self._b)
        elif lib.lpcnet_batch_reset_stream(self._b, stream) != 0:
            raise LPCNetError(last_error())

    def synthesize(self, features: np.ndarray, n: int = FRAME_SIZE) -> np.ndarray:
        """features [B, >=20] -> pcm [B, n] int16 (one frame per stream)."""
        f = np.ascontiguousarray(np.asarray(features, np.float32)[:, :NB_FEATURES])
        assert f.shape[0] == self.B
        out = np.zeros((self.B, n), np.int16)
        if lib.lpcnet_batch_synthesize(self._b, f.ctypes.data, out.ctypes.data, n) != 0:
            raise LPCNetError(last_error())
        return out

    def host_features(self) -> np.ndarray:
        """The batch's feature buffer [B, 20] (lpcnet_batch_host_features:
        host-visible VRAM on large-BAR devices, else pinned host memory;
        write-combined there, so fill it in place and do not read it back
        in a hot loop), then synthesize_host()."""
        if getattr(self, "_hf", None) is None:
            p = lib.lpcnet_batch_host_features(self._b)
            if not p:
                raise LPCNetError(last_error())
            self._hf = _owned_view(self._owner, C.cast(p, C.c_void_p).value, C.c_float, np.float32, (self.B, NB_FEATURES))
            q = lib.lpcnet_batch_host_pcm(self._b)
            if not q:
                raise LPCNetError(last_error())
            self._hp = _owned_view(self._owner, C.cast(q, C.c_void_p).value, C.c_int16, np.int16, (self.B * FRAME_SIZE,))
            # the live tick's arguments, resolved once (ctypes attribute
            # lookups per call are microseconds of host turn-around)
            self._hf_addr, self._hp_addr = self._hf.ctypes.data, self._hp.ctypes.data
        return self._hf

    def synthesize_host(self, n: int = FRAME_SIZE) -> np.ndarray:
        """One frame from host_features() into the batch's pinned PCM buffer
        (lpcnet_batch_synthesize on the batch's own buffers: no host staging
        copies; the sample kernel stores the PCM there itself where it can).
        Returns a [B, n] view of that buffer, overwritten by the next call
        (copy it to keep it); the view keeps the batch's host buffers alive
        past close()."""
        self.host_features()
        if lib.lpcnet_batch_synthesize(self._b, self._hf_addr, self._hp_addr, n) != 0:
            raise LPCNetError(last_error())
        return self._hp[:self.B * n].reshape(self.B, n)

    def synthesize_impl(self, features: np.ndarray, pcm: np.ndarray, preload: int) -> np.ndarray:
        """lpcnet_synthesize_impl: pcm [B, N] int16, first ``preload`` samples teacher-forced."""
        f = np.ascontiguousarray(np.asarray(features, np.float32)[:, :NB_FEATURES])
        out = np.ascontiguousarray(pcm, np.int16).copy()
        n = out.shape[1] if out.ndim == 2 else 0
        if lib.lpcnet_batch_synthesize_impl(self._b, f.ctypes.data, out.ctypes.data if n else None, n, preload) != 0:
            raise LPCNetError(last_error())
        return out

    def frame_only(self, features: np.ndarray) -> None:
        """run_frame_network without samples (lpcnet.c:134 run_frame_network_flush)."""
        f = np.ascontiguousarray(np.asarray(features, np.float32)[:, :NB_FEATURES])
        if lib.lpcnet_batch_synthesize_impl(self._b, f.ctypes.data, None, 0, 0) != 0:
            raise LPCNetError(last_error())

    def synthesize_tail_impl(self, pcm: np.ndarray, preload: int = 0) -> np.ndarray:
        """lpcnet_synthesize_tail_impl on every stream: pcm [B, N] (first ``preload`` teacher-forced)."""
        out = np.ascontiguousarray(pcm, np.int16).copy()
        n = out.shape[1]
        if lib.lpcnet_batch_synthesize_tail_impl(self._b, out.ctypes.data if n else None, n, preload) != 0:
            raise LPCNetError(last_error())
        return out

    def run_frame_network(self, features: np.ndarray, update_conditions: bool) -> None:
        """run_frame_network of one frame per stream; update_conditions False = flush semantics."""
        f = np.ascontiguousarray(np.asarray(features, np.float32)[:, :NB_FEATURES])
        if lib.lpcnet_batch_run_frame_network(self._b, f.ctypes.data, 1 if update_conditions else 0) != 0:
            raise LPCNetError(last_error())

    def reset_signal(self, stream: int) -> None:
        if lib.lpcnet_batch_reset_signal(self._b, stream) != 0:
            raise LPCNetError(last_error())

    def decode(self, packets: np.ndarray) -> np.ndarray:
        """lpcnet_decode on every stream: packets [B, 8] uint8 -> pcm [B, 640]."""
        pk = np.ascontiguousarray(packets, np.uint8)
        assert pk.shape == (self.B, 8)
        out = np.zeros((self.B, 4 * FRAME_SIZE), np.int16)
        if lib.lpcnet_batch_decode(self._b, pk.ctypes.data, out.ctypes.data) != 0:
            raise LPCNetError(last_error())
        return out

    def decode_frames(self, d_packets: int, d_pcm: int, npackets: int) -> None:
        """Enqueue device packets [npackets, B, 8] -> device pcm [4 npackets, B, 160]."""
        if lib.lpcnet_batch_decode_frames(self._b, d_packets, d_pcm, npackets) != 0:
            raise LPCNetError(last_error())

    def save_state(self, stream: int) -> bytes:
        return _save_snapshot(lib.lpcnet_batch_save_state, self._b, stream, lib.lpcnet_batch_state_size())

    def restore_state(self, stream: int, state: bytes) -> None:
        if lib.lpcnet_batch_restore_state(self._b, stream, state) != 0:
            raise LPCNetError(last_error())

    # -- PLC prediction network (compute_plc_pred, lpcnet_plc.c:135-145) ------
    def plc_info(self) -> tuple[int, int, int, int]:
        """(57, cond, units1, units2) of the loaded model's predictor."""
        d = (C.c_int * 4)()
        if lib.lpcnet_batch_plc_info(self._b, d) != 0:
            raise LPCNetError(last_error())
        return tuple(d)

    def plc_predict(self, inputs: np.ndarray | None = None, active: np.ndarray | None = None,
                    out: np.ndarray | None = None, discard: bool = False) -> np.ndarray | None:
        """compute_plc_pred on every stream with active[s] != 0 (None: all).
        inputs [B, 57] (None: the all-zero concealment input); returns
        [B, 20] features -- rows of inactive streams keep what ``out`` held
        (zeros without ``out``) -- or None with discard=True."""
        x = None if inputs is None else np.ascontiguousarray(inputs, np.float32)
        if x is not None and x.shape != (self.B, PLC_INPUTS):
            raise ValueError(f"inputs must be [{self.B}, {PLC_INPUTS}]")
        a = _active_arg(active, self.B)
        o = None if discard else _out_arg(out, (self.B, NB_FEATURES))
        if lib.lpcnet_batch_plc_predict(self._b, _ptr(x), _ptr(o), _ptr(a)) != 0:
            raise LPCNetError(last_error())
        return o

    def plc_predict_device(self, d_in: int | None, d_out: int | None, d_active: int | None = None) -> None:
        """Enqueue the predictor on device buffers: d_in [B, 57] (None: zeros),
        d_out [B, 20] (None: discard; the layout synthesize_frames reads as
        d_features), d_active [B] bytes (None: all).  sync() waits."""
        if lib.lpcnet_batch_plc_predict_device(self._b, d_in, d_out, d_active) != 0:
            raise LPCNetError(last_error())

    def plc_reset(self, stream: int | None = None) -> None:
        """Zero the predictor state of one stream (None: all), as lpcnet_plc_reset does."""
        if lib.lpcnet_batch_plc_reset(self._b, -1 if stream is None else stream) != 0:
            raise LPCNetError(last_error())

    def plc_save_state(self, stream: int) -> bytes:
        """plc_gru1_state | plc_gru2_state of one stream (the PLC's PLCNetState copies)."""
        return _save_snapshot(lib.lpcnet_batch_plc_save_state, self._b, stream, lib.lpcnet_batch_plc_state_size(self._b))

    def plc_restore_state(self, stream: int, state: bytes) -> None:
        _restore_snapshot(lib.lpcnet_batch_plc_restore_state, self._b, stream, state, lib.lpcnet_batch_plc_state_size(self._b),
                          last_error() or "PLC state of the wrong size")  # the size call's error, when it left one

    # -- DRED RDO-VAE (dred_rdovae_enc.c, dred_rdovae_dec.c, dred_rdovae.c) ----
    def rdovae_info(self) -> dict:
        """rdovae_dims of the loaded model."""
        d = (C.c_int * 24)()
        if lib.lpcnet_batch_rdovae_info(self._b, d) != 0:
            raise LPCNetError(last_error())
        return _rdovae_dims_dict(d)

    def _rdovae_side(self, side: str) -> dict:
        d = self.rdovae_info()[side]
        if d is None:  # the reason is the size call's
            lib.lpcnet_batch_rdovae_state_size(self._b, 1 if side == "enc" else 2)
            raise LPCNetError(last_error())
        return d

    def rdovae_encode(self, inputs: np.ndarray, active: np.ndarray | None = None, latents: np.ndarray | None = None,
                      state: np.ndarray | None = None) -> tuple[np.ndarray, np.ndarray]:
        """dred_rdovae_encode_dframe on every stream with active[s] != 0 (None:
        all): inputs [B, 40], two consecutive 20-feature frames, the earlier
        first -> (latents [B, L], initial state [B, S]).  Rows of inactive
        streams keep what ``latents`` / ``state`` held (zeros without them)."""
        d = self._rdovae_side("enc")
        x = np.ascontiguousarray(inputs, np.float32)
        if x.shape != (self.B, 2 * NB_FEATURES):
            raise ValueError(f"inputs must be [{self.B}, {2 * NB_FEATURES}]")
        a = _active_arg(active, self.B)
        z = _out_arg(latents, (self.B, d["L"]), what="latents")
        st = _out_arg(state, (self.B, d["S"]), what="state")
        if lib.lpcnet_batch_rdovae_encode(self._b, _ptr(x), _ptr(z), _ptr(st), _ptr(a)) != 0:
            raise LPCNetError(last_error())
        return z, st

    def rdovae_encode_device(self, d_features: int | None, d_latents: int | None, d_state: int | None, row: int = NB_FEATURES,
                             d_active: int | None = None) -> None:
        """Enqueue the encoder on device buffers: d_features [2, B, row], row 20
        or 36 (what compute_features_device writes for two frames), d_latents
        [B, L], d_state [B, S].  sync() waits."""
        if lib.lpcnet_batch_rdovae_encode_device(self._b, d_features, row, d_latents, d_state, d_active) != 0:
            raise LPCNetError(last_error())

    def rdovae_dec_init(self, state: np.ndarray, active: np.ndarray | None = None) -> None:
        """dred_rdovae_dec_init_states: state [B, S] -> the streams' decoder state."""
        d = self._rdovae_side("dec")
        st = np.ascontiguousarray(state, np.float32)
        if st.shape != (self.B, d["S"]):
            raise ValueError(f"state must be [{self.B}, {d['S']}]")
        a = _active_arg(active, self.B)
        if lib.lpcnet_batch_rdovae_dec_init(self._b, _ptr(st), _ptr(a)) != 0:
            raise LPCNetError(last_error())

    def rdovae_dec_init_device(self, d_state: int | None, d_active: int | None = None) -> None:
        if lib.lpcnet_batch_rdovae_dec_init_device(self._b, d_state, d_active) != 0:
            raise LPCNetError(last_error())

    def rdovae_decode_qframe(self, latents: np.ndarray, active: np.ndarray | None = None,
                             out: np.ndarray | None = None) -> np.ndarray:
        """dred_rdovae_decode_qframe on the streams' decoder state: latents
        [B, L] -> [B, 80], four feature frames in reverse order."""
        d = self._rdovae_side("dec")
        z = np.ascontiguousarray(latents, np.float32)
        if z.shape != (self.B, d["L"]):
            raise ValueError(f"latents must be [{self.B}, {d['L']}]")
        a = _active_arg(active, self.B)
        o = _out_arg(out, (self.B, 4 * NB_FEATURES))
        if lib.lpcnet_batch_rdovae_decode_qframe(self._b, _ptr(z), _ptr(o), _ptr(a)) != 0:
            raise LPCNetError(last_error())
        return o

    def rdovae_decode_qframe_device(self, d_latents: int | None, d_qframe: int | None, d_active: int | None = None) -> None:
        if lib.lpcnet_batch_rdovae_decode_qframe_device(self._b, d_latents, d_qframe, d_active) != 0:
            raise LPCNetError(last_error())

    def rdovae_decode_all(self, state: np.ndarray, latents: np.ndarray, active: np.ndarray | None = None,
                          out: np.ndarray | None = None) -> np.ndarray:
        """DRED_rdovae_decode_all: state [B, S], latents [B, n, L] -> features
        [B, 4 n, 20] in the reference's own order, on a temporary state (the
        streams' decoder state is untouched)."""
        d = self._rdovae_side("dec")
        st = np.ascontiguousarray(state, np.float32)
        z = np.ascontiguousarray(latents, np.float32)
        if st.shape != (self.B, d["S"]):
            raise ValueError(f"state must be [{self.B}, {d['S']}]")
        if z.ndim != 3 or z.shape[0] != self.B or z.shape[2] != d["L"]:
            raise ValueError(f"latents must be [{self.B}, n, {d['L']}]")
        n = z.shape[1]
        a = _active_arg(active, self.B)
        o = _out_arg(out, (self.B, 4 * n, NB_FEATURES))
        if lib.lpcnet_batch_rdovae_decode_all(self._b, _ptr(st), _ptr(z), _ptr(o), n, _ptr(a)) != 0:
            raise LPCNetError(last_error())
        return o

    def rdovae_decode_all_device(self, d_state: int | None, d_latents: int | None, d_features: int | None, n: int,
                                 d_active: int | None = None) -> None:
        """Enqueue decode_all on device buffers: d_state [B, S], d_latents
        [B, n, L], d_features [B, 4 n, 20].  sync() waits."""
        if lib.lpcnet_batch_rdovae_decode_all_device(self._b, d_state, d_latents, d_features, n, d_active) != 0:
            raise LPCNetError(last_error())

    def rdovae_reset(self, stream: int | None = None, which: int = 3) -> None:
        """Zero the RDO-VAE state of one stream (None: all): which = 1 the
        encoder's, 2 the decoder's, 3 both."""
        if lib.lpcnet_batch_rdovae_reset(self._b, -1 if stream is None else stream, which) != 0:
            raise LPCNetError(last_error())

    def rdovae_save_state(self, stream: int, which: int = 3) -> bytes:
        """The GRU states dense2 | dense4 | dense6 and, for the encoder, the
        conv memory of one stream (which as rdovae_reset; both: the encoder's first)."""
        save = lambda b, s, buf: lib.lpcnet_batch_rdovae_save_state(b, s, which, buf)
        return _save_snapshot(save, self._b, stream, lib.lpcnet_batch_rdovae_state_size(self._b, which))

    def rdovae_restore_state(self, stream: int, state: bytes, which: int = 3) -> None:
        restore = lambda b, s, buf: lib.lpcnet_batch_rdovae_restore_state(b, s, which, buf)
        _restore_snapshot(restore, self._b, stream, state, lib.lpcnet_batch_rdovae_state_size(self._b, which),
                          last_error() or "RDO-VAE state of the wrong size")  # the size call's error, when it left one

    # -- feature extraction (lpcnet_compute_single_frame_features) ----------
    def compute_features(self, pcm: np.ndarray, active: np.ndarray | None = None,
                         out: np.ndarray | None = None) -> np.ndarray:
        """preemphasis + compute_frame_features + process_single_frame on every
        stream with active[s] != 0 (None: all).  pcm [B, 160], int16 or float32
        (the reference's short -> float conversion already done); returns
        [B, 36] features -- rows of inactive streams keep what ``out`` held
        (zeros without ``out``).  Needs no model."""
        p = _pcm_arg(pcm, (self.B, FRAME_SIZE), float_ok=True)
        a = _active_arg(active, self.B)
        o = _out_arg(out, (self.B, NB_TOTAL_FEATURES))
        fn = lib.lpcnet_batch_compute_features if p.dtype == np.int16 else lib.lpcnet_batch_compute_features_float
        if fn(self._b, _ptr(p), _ptr(o), _ptr(a)) != 0:
            raise LPCNetError(last_error())
        return o

    def compute_features_device(self, d_pcm: int, d_features: int, row: int = NB_FEATURES,
                                d_active: int | None = None, nframes: int = 1) -> None:
        """Enqueue the extractor on device buffers: d_pcm [nframes, B, 160] int16
        (what synthesize_frames writes), d_features [nframes, B, row] with row
        20 (what synthesize_frames reads as d_features) or 36,
        d_active [B] bytes (None: all).  sync() waits."""
        if lib.lpcnet_batch_compute_features_device(self._b, d_pcm, d_features, row, d_active, nframes) != 0:
            raise LPCNetError(last_error())

    def features_reset(self, stream: int | None = None) -> None:
        """Zero the analysis state of one stream (None: all), as lpcnet_encoder_init does."""
        if lib.lpcnet_batch_features_reset(self._b, -1 if stream is None else stream) != 0:
            raise LPCNetError(last_error())

    def features_save_state(self, stream: int) -> bytes:
        return _save_snapshot(lib.lpcnet_batch_features_save_state, self._b, stream, lib.lpcnet_batch_features_state_size(self._b))

    def features_restore_state(self, stream: int, state: bytes) -> None:
        _restore_snapshot(lib.lpcnet_batch_features_restore_state, self._b, stream, state,
                          lib.lpcnet_batch_features_state_size(self._b), "analysis state of the wrong size")

    # -- Burg cepstral analysis and the predictor's input rows ---------------
    def burg_cepstrum(self, pcm: np.ndarray, active: np.ndarray | None = None,
                      out: np.ndarray | None = None) -> np.ndarray:
        """burg_cepstral_analysis on every stream with active[s] != 0 (None:
        all).  pcm [B, 160], int16 or float32; returns [B, 36] -- rows of
        inactive streams keep what ``out`` held (zeros without ``out``).
        Needs no model and has no state."""
        p = _pcm_arg(pcm, (self.B, FRAME_SIZE), float_ok=True)
        a = _active_arg(active, self.B)
        o = _out_arg(out, (self.B, BURG_CEPSTRUM))
        fn = lib.lpcnet_batch_burg_cepstrum if p.dtype == np.int16 else lib.lpcnet_batch_burg_cepstrum_float
        if fn(self._b, _ptr(p), _ptr(o), _ptr(a)) != 0:
            raise LPCNetError(last_error())
        return o

    def burg_cepstrum_device(self, d_pcm: int, d_out: int, row: int = BURG_CEPSTRUM, col: int = 0,
                             d_active: int | None = None, nframes: int = 1) -> None:
        """Enqueue the Burg analysis on device buffers: d_pcm [nframes, B, 160]
        int16, the 36 values of frame f and stream s at
        d_out[(f * B + s) * row + col]; row >= col + 36.  sync() waits."""
        if lib.lpcnet_batch_burg_cepstrum_device(self._b, d_pcm, d_out, row, col, d_active, nframes) != 0:
            raise LPCNetError(last_error())

    def plc_rows_device(self, d_pcm: int, d_rows: int, parts: int = PLC_ROW_BURG | PLC_ROW_FEATURES, flag: float = 1.0,
                        d_active: int | None = None) -> None:
        """Enqueue the assembly of one predictor input row [B, 57] per active
        stream from d_pcm [B, 160] int16: the Burg cepstrum (PLC_ROW_BURG),
        the extractor's 20 features (PLC_ROW_FEATURES; advances the analysis
        state), zeros in an unselected part, ``flag`` in column 56."""
        if lib.lpcnet_batch_plc_rows_device(self._b, d_pcm, d_rows, parts, flag, d_active) != 0:
            raise LPCNetError(last_error())

    def plc_update(self, pcm: np.ndarray, active: np.ndarray | None = None, out: np.ndarray | None = None) -> np.ndarray:
        """The PLC's good-packet step on every stream with active[s] != 0:
        pcm [B, 160] int16 -> rows(Burg | features, flag 1) -> compute_plc_pred
        -> [B, 20].  Rows of inactive streams keep what ``out`` held."""
        p = _pcm_arg(pcm, (self.B, FRAME_SIZE))
        a = _active_arg(active, self.B)
        o = _out_arg(out, (self.B, NB_FEATURES))
        if lib.lpcnet_batch_plc_update(self._b, _ptr(p), _ptr(o), _ptr(a)) != 0:
            raise LPCNetError(last_error())
        return o

    def plc_update_device(self, d_pcm: int, d_out: int, d_active: int | None = None) -> None:
        """plc_update on device buffers: d_pcm [B, 160] int16, d_out [B, 20]
        (what synthesize_frames reads as d_features).  sync() waits."""
        if lib.lpcnet_batch_plc_update_device(self._b, d_pcm, d_out, d_active) != 0:
            raise LPCNetError(last_error())

    # -- 1.6 kb/s encoder (lpcnet_encode, lpcnet_compute_features) ----------
    def encode(self, pcm: np.ndarray, active: np.ndarray | None = None, packets: np.ndarray | None = None,
               features: np.ndarray | None = None, want_features: bool = True):
        """lpcnet_encode on every stream with active[s] != 0 (None: all): pcm
        [B, 640] int16 -> (packets [B, 8] uint8, features [4, B, 36] or None):
        st->features after quantisation.  Rows of inactive streams keep what
        ``packets`` / ``features`` held (zeros without them).  Needs a model
        with the ceps codebooks."""
        p = _pcm_arg(pcm, (self.B, 4 * FRAME_SIZE))
        a = _active_arg(active, self.B)
        pk = _out_arg(packets, (self.B, 8), np.uint8, "packets")
        f = None
        if want_features or features is not None:
            f = _out_arg(features, (4, self.B, NB_TOTAL_FEATURES), what="features")
        if lib.lpcnet_batch_encode(self._b, _ptr(p), _ptr(pk), _ptr(f), _ptr(a)) != 0:
            raise LPCNetError(last_error())
        return pk, f

    def compute_features4(self, pcm: np.ndarray, active: np.ndarray | None = None,
                          out: np.ndarray | None = None) -> np.ndarray:
        """lpcnet_compute_features (unquantised): pcm [B, 640] int16 ->
        features [4, B, 36].  Needs no model."""
        p = _pcm_arg(pcm, (self.B, 4 * FRAME_SIZE))
        a = _active_arg(active, self.B)
        o = _out_arg(out, (4, self.B, NB_TOTAL_FEATURES), what="features")
        if lib.lpcnet_batch_compute_features4(self._b, _ptr(p), _ptr(o), _ptr(a)) != 0:
            raise LPCNetError(last_error())
        return o

    def encode_device(self, d_pcm: int, d_packets: int, d_features: int | None = None, row: int = NB_FEATURES,
                      d_active: int | None = None, npackets: int = 1) -> None:
        """Enqueue the encoder on device buffers: d_pcm [4 npackets, B, 160]
        int16 (what synthesize_frames writes), d_packets [npackets, B, 8] (what
        decode_frames reads), d_features [4 npackets, B, row] or None, row 20
        or 36.  sync() waits."""
        if lib.lpcnet_batch_encode_device(self._b, d_pcm, d_packets, d_features, row, d_active, npackets) != 0:
            raise LPCNetError(last_error())

    def encode_save_state(self, stream: int) -> bytes:
        """The features snapshot followed by the encoder's vq_mem[18]."""
        return _save_snapshot(lib.lpcnet_batch_encode_save_state, self._b, stream, lib.lpcnet_batch_encode_state_size(self._b))

    def encode_restore_state(self, stream: int, state: bytes) -> None:
        _restore_snapshot(lib.lpcnet_batch_encode_restore_state, self._b, stream, state,
                          lib.lpcnet_batch_encode_state_size(self._b), "encoder state of the wrong size")

    # -- concealment machine (lpcnet_plc_update / lpcnet_plc_conceal) --------
    def conceal_open(self, options: int = CONCEAL_CAUSAL) -> None:
        """lpcnet_plc_init + lpcnet_plc_reset for every stream: CONCEAL_CAUSAL,
        CONCEAL_NONCAUSAL or CONCEAL_CODEC, with or without CONCEAL_DC_FILTER.
        Needs a model with PLC records; CONCEAL_NONCAUSAL also FEATURES_DELAY 0
        (set_model_constants or the blob's record)."""
        if lib.lpcnet_batch_conceal_open(self._b, options) != 0:
            raise LPCNetError(last_error())

    def conceal_close(self) -> None:
        if lib.lpcnet_batch_conceal_close(self._b) != 0:
            raise LPCNetError(last_error())

    def conceal_reset(self, stream: int | None = None) -> None:
        """lpcnet_plc_reset of one stream (None: all)."""
        if lib.lpcnet_batch_conceal_reset(self._b, -1 if stream is None else stream) != 0:
            raise LPCNetError(last_error())

    def _lost_arg(self, lost) -> np.ndarray:
        lo = np.ascontiguousarray(np.asarray(lost) != 0, np.uint8)
        if lo.shape != (self.B,):
            raise ValueError(f"lost must be [{self.B}]")
        return lo

    def conceal_frame(self, pcm: np.ndarray, lost, active=None) -> np.ndarray:
        """One tick: stream s with lost[s] == 0 runs lpcnet_plc_update on
        pcm[s], with lost[s] != 0 lpcnet_plc_conceal into it.  pcm [B, 160]
        int16; returns the PCM after the tick (rows of inactive streams as
        given)."""
        p = _pcm_arg(pcm, (self.B, FRAME_SIZE)).copy()
        lo, a = self._lost_arg(lost), _active_arg(active, self.B)
        if lib.lpcnet_batch_conceal_frame(self._b, _ptr(p), _ptr(lo), _ptr(a)) != 0:
            raise LPCNetError(last_error())
        return p

    def conceal_frame_device(self, d_pcm: int, lost, active=None) -> None:
        """conceal_frame on device PCM [B, 160] int16, in place and queued:
        sync() waits.  lost / active are read during the call."""
        lo, a = self._lost_arg(lost), _active_arg(active, self.B)
        if lib.lpcnet_batch_conceal_frame_device(self._b, d_pcm, _ptr(lo), _ptr(a)) != 0:
            raise LPCNetError(last_error())

    def conceal_fec_add(self, stream: int, features: np.ndarray | None) -> None:
        """lpcnet_plc_fec_add: features [>= 20], or None for a frame without FEC (fec_skip++)."""
        f = None if features is None else np.ascontiguousarray(np.asarray(features, np.float32).ravel()[:NB_FEATURES])
        if f is not None and f.size != NB_FEATURES:
            raise ValueError("features must hold 20 values")
        if lib.lpcnet_batch_conceal_fec_add(self._b, stream, _ptr(f)) != 0:
            raise LPCNetError(last_error())

    def conceal_fec_clear(self, stream: int) -> None:
        if lib.lpcnet_batch_conceal_fec_clear(self._b, stream) != 0:
            raise LPCNetError(last_error())

    def conceal_state(self, stream: int) -> dict:
        """The machine's state of one stream: the control fields (CONCEAL_CTRL),
        features [20], pcm [FEATURES_DELAY * 160 + 240] int16, dc_mem, syn_dc."""
        ctrl = np.zeros(len(CONCEAL_CTRL), np.int32)
        f = np.zeros(NB_FEATURES, np.float32)
        p = np.zeros(4 * FRAME_SIZE + 240, np.int16)  # the largest FEATURES_DELAY
        dc = np.zeros(2, np.float64)
        if lib.lpcnet_batch_conceal_get_state(self._b, stream, ctrl.ctypes.data, f.ctypes.data, p.ctypes.data, dc.ctypes.data) != 0:
            raise LPCNetError(last_error())
        out = dict(zip(CONCEAL_CTRL, (int(v) for v in ctrl)))
        out.update(features=f, pcm=p[:self.info().features_delay * FRAME_SIZE + 240].copy(), dc_mem=float(dc[0]), syn_dc=float(dc[1]))
        return out

    def conceal_state_noncausal(self, stream: int) -> dict:
        """What the non-causal mode keeps beside conceal_state(): queued_update,
        queued_samples [160] int16, dc_buf [80] int16.  LPCNetError when the
        open machine is in another mode."""
        q = C.c_int(0)
        qs = np.zeros(FRAME_SIZE, np.int16)
        db = np.zeros(FRAME_SIZE // 2, np.int16)
        if lib.lpcnet_batch_conceal_get_state_noncausal(self._b, stream, C.addressof(q), qs.ctypes.data, db.ctypes.data) != 0:
            raise LPCNetError(last_error())
        return {"queued_update": int(q.value), "queued_samples": qs, "dc_buf": db}

    # -- device-resident path (benchmarks) ---------------------------------
    def device_alloc(self, nbytes: int) -> int:
        p = lib.lpcnet_batch_device_alloc(self._b, nbytes)
        if not p:
            raise LPCNetError(last_error())
        return p

    def device_free(self, p: int) -> None:
        lib.lpcnet_batch_device_free(self._b, p)

    def h2d(self, dst: int, arr: np.ndarray) -> None:
        a = np.ascontiguousarray(arr)
        if lib.lpcnet_batch_memcpy_h2d(self._b, dst, a.ctypes.data, a.nbytes) != 0:
            raise LPCNetError(last_error())

    def d2h(self, arr: np.ndarray, src: int) -> None:
        if lib.lpcnet_batch_memcpy_d2h(self._b, arr.ctypes.data, src, arr.nbytes) != 0:
            raise LPCNetError(last_error())

    def synthesize_frames(self, h_features: np.ndarray, d_features: int, d_pcm: int, nframes: int,
                          n: int = FRAME_SIZE) -> None:
        """Enqueue ``nframes`` frames from device features [nframes, B, 20] into device pcm
        [nframes, B, n].  ``h_features`` is unused (LPC runs on the device); kept for callers."""
        if lib.lpcnet_batch_synthesize_frames(self._b, None, d_features, d_pcm, nframes, n) != 0:
            raise LPCNetError(last_error())

    def sync(self) -> None:
        if lib.lpcnet_batch_sync(self._b) != 0:
            raise LPCNetError(last_error())

    def reset_timers(self, enable: bool | int = True) -> None:
        """0/False off, 1 sample kernel only, 2/True sample and frame kernels."""
        lib.lpcnet_batch_reset_timers(self._b, 2 if enable is True else int(enable))

    def kernel_ms(self, which: int = 0) -> tuple[float, int]:
        """(total ms, launches) of the timed launches since reset_timers: which = 0 sample
        kernel, 1 frame kernel, 2 PLC predictor, 3 feature extractor, 4 the 1.6 kb/s
        encoder, 5 the part of 4 that is enc_kernel.hip, 6 the Burg analysis, 8 the
        RDO-VAE encoder, 9 the RDO-VAE decoder (7 is no region)."""
        n = C.c_int(0)
        ms = lib.lpcnet_batch_kernel_ms(self._b, which, C.byref(n))
        return ms, n.value

    def kernel_frames(self, which: int = 0) -> int:
        """Frames covered by the timed launches (multi-frame launches count each frame)."""
        return lib.lpcnet_batch_kernel_frames(self._b, which)

    def set_stamps(self, enable: bool = True) -> None:
        if lib.lpcnet_batch_set_stamps(self._b, 1 if enable else 0) != 0:
            raise LPCNetError(last_error())

    def get_stamps(self) -> np.ndarray:
        """[workgroups, 8 waves, 16] s_memtime sums of the last sample-kernel launch."""
        out = np.zeros((self.B, 8, 16), np.uint64)
        g = lib.lpcnet_batch_get_stamps(self._b, out.ctypes.data)
        if g < 0:
            raise LPCNetError("stamps not enabled")
        return out[:g]

    def get_frame_stamps(self) -> np.ndarray:
        """[workgroups, 16] s_memtime phase durations of the last frame-kernel launch."""
        out = np.zeros((self.B, 16), np.uint64)  # >= the frame kernel's workgroups for any batch
        g = lib.lpcnet_batch_get_frame_stamps(self._b, out.ctypes.data)
        if g < 0:
            raise LPCNetError("stamps not enabled")
        return out[:g]

    def set_trace(self, enable: bool = True) -> None:
        lib.lpcnet_batch_set_trace(self._b, 1 if enable else 0)

    def get_trace(self, n: int) -> tuple[np.ndarray, np.ndarray]:
        logits = np.zeros((self.B, n, 8), np.float32)
        exc = np.zeros((self.B, n), np.int32)
        if lib.lpcnet_batch_get_trace(self._b, logits.ctypes.data, exc.ctypes.data) != 0:
            raise LPCNetError("trace not enabled")
        return logits, exc

    def get_state(self, stream: int) -> dict:
        a = np.zeros(1152, np.float32)
        b = np.zeros(48, np.float32)
        lpc = np.zeros(16, np.float32)
        sa = np.zeros(384, np.float32)
        sb = np.zeros(16, np.float32)
        fc = C.c_int(0)
        if lib.lpcnet_batch_get_state(self._b, stream, a.ctypes.data, b.ctypes.data, lpc.ctypes.data,
                                      sa.ctypes.data, sb.ctypes.data, C.byref(fc)) != 0:
            raise LPCNetError(last_error())
        return {"gru_a_cond": a, "gru_b_cond": b, "lpc": lpc, "gru_a_state": sa, "gru_b_state": sb,
                "frame_count": fc.value}

    def close(self) -> None:
        """Release the batch: destroyed now, or when the last array handed
        out by host_features() / synthesize_host() goes."""
        if self._b:
            self._hf = self._hp = None
            self._b = None
            self._owner = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
