"""CPU restatement of burg_cepstral_analysis (freq.c:156-199) and
silk_burg_analysis (burg.c:98-245) in numpy float32 / Python float (an IEEE
double) scalars, with an explicit cast wherever the C types round: what
burg_kernel.hip restates on the device.  The 320-point kiss FFT (factors
4, 4, 4, 5) is restated here too, vectorised over its independent
butterflies (elementwise float32 numpy arithmetic rounds every product and
sum on its own, as the reference's build without contraction does), so the
fixture tests need no compiled reference.  Also the fixture's signals and
loader, and the ctypes view of the compiled reference (oracle/_ref) the
fixture's maker and the live tests share.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

import feat_signals as FS
import oracle_lib as O

F = np.float32
FRAME_SIZE = 160
HALF = 80
NB_BANDS = 18
LPC_ORDER = 16
WINDOW_SIZE = 320
BURG_LEN = HALF - 1          # freq.c:170: len - 1 samples
PREEMPHASIS = F(0.85)        # freq.h:34
COND_FAC = float(F(1e-5))    # burg.c:40 FIND_LPC_COND_FAC, a float literal promoted to double
MIN_INV_GAIN = float(F(1e-3))  # a float parameter (burg.c:101, freq.c:170)
EBAND = [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 34, 40]  # freq.c:45-48
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "burg_cepstrum.npz")

# the four sine signals of the fixture: name -> (normalised frequencies, amplitude)
SINES = {"sine1": ((.031,), 12000), "sine2": ((.031, .117), 8000), "sine3": ((.031, .117, .29), 6000),
         "sine5": ((.02, .07, .13, .21, .33), 5000)}
NAMES = FS.NAMES + list(SINES)


def make_sine(name: str) -> np.ndarray:
    """[3840] int16: rint(sum_i amp sin(2 pi f_i n + 0.3 i))."""
    freqs, amp = SINES[name]
    n = np.arange(FS.N)
    return np.rint(sum(amp * np.sin(2 * np.pi * f * n + 0.3 * i) for i, f in enumerate(freqs))).astype(np.int16)


_fix = None


def fixture() -> dict:
    """The committed fixture, read-only: names, pcm_sine [4, 24, 160] int16,
    ceps [33, 24, 36], A [33, 24, 2, 16], nrg [33, 24, 2] float32,
    stop_order [33, 24, 2] int32."""
    global _fix
    if _fix is None:
        with np.load(GOLDEN) as g:
            _fix = {k: g[k] for k in g.files}
        for v in _fix.values():
            v.setflags(write=False)
    return _fix


def pcm_of(name: str) -> np.ndarray:
    """[24, 160] of one signal, int16 or float32: the 29 extractor signals from
    their own fixture, the sines from this one."""
    if name in SINES:
        return fixture()["pcm_sine"][list(SINES).index(name)]
    return FS.pcm_of(name)


def stop_from_A(A: np.ndarray) -> int:
    """The order at which the recursion hit the gain clamp, from the
    coefficients alone: the clamp zeroes every coefficient after its own.
    0: all zero; 16: never (or at the last order)."""
    nz = np.flatnonzero(np.asarray(A) != 0)
    return 0 if not nz.size else int(nz[-1]) + 1


# -- silk_burg_analysis ---------------------------------------------------------

def _inner(a, b, n: int) -> float:
    """silk_energy_FLP / silk_inner_product_FLP (burg.c:43-94) on lists of
    Python floats: double products, result += ((p0+p1)+p2)+p3, the remainder
    one by one."""
    result = 0.0
    i = 0
    while i < n - 3:
        result += a[i] * b[i] + a[i + 1] * b[i + 1] + a[i + 2] * b[i + 2] + a[i + 3] * b[i + 3]
        i += 4
    while i < n:
        result += a[i] * b[i]
        i += 1
    return result


def silk_burg(x32: np.ndarray, D: int = LPC_ORDER):
    """silk_burg_analysis(A, x, (float)1e-3, len(x), 1, D): (A [D] float32,
    residual energy float32, stop order)."""
    L = len(x32)
    x = [float(v) for v in x32]  # exact
    C0 = _inner(x, x, L)
    Cf = [_inner(x, x[n:], L - n) for n in range(1, D + 1)]
    Cl = list(Cf)
    CAf = [0.0] * (D + 1)
    CAb = [0.0] * (D + 1)
    Af = [0.0] * D
    CAb[0] = CAf[0] = C0 + COND_FAC * C0 + float(F(1e-9))
    invGain = 1.0
    reached = False
    stop = D
    for n in range(D):
        tmp1 = x[n]
        tmp2 = x[L - n - 1]
        for k in range(n):
            # float products, rounded to float before the double subtraction
            Cf[k] -= float(x32[n] * x32[n - k - 1])
            Cl[k] -= float(x32[L - n - 1] * x32[L - n + k])
            Atmp = Af[k]
            tmp1 += x[n - k - 1] * Atmp
            tmp2 += x[L - n + k] * Atmp
        for k in range(n + 1):
            CAf[k] -= tmp1 * x[n - k]
            CAb[k] -= tmp2 * x[L - n + k - 1]
        tmp1 = Cf[n]
        tmp2 = Cl[n]
        for k in range(n):
            Atmp = Af[k]
            tmp1 += Cl[n - k - 1] * Atmp
            tmp2 += Cf[n - k - 1] * Atmp
        CAf[n + 1] = tmp1
        CAb[n + 1] = tmp2
        num = CAb[n + 1]
        nrg_b = CAb[0]
        nrg_f = CAf[0]
        for k in range(n):
            Atmp = Af[k]
            num += CAb[n - k] * Atmp
            nrg_b += CAb[k + 1] * Atmp
            nrg_f += CAf[k + 1] * Atmp
        rc = -2.0 * num / (nrg_f + nrg_b)
        tmp1 = invGain * (1.0 - rc * rc)
        if tmp1 <= MIN_INV_GAIN:
            rc = math.sqrt(1.0 - MIN_INV_GAIN / invGain)
            if num > 0:
                rc = -rc
            invGain = MIN_INV_GAIN
            reached = True
        else:
            invGain = tmp1
        for k in range((n + 1) >> 1):
            tmp1 = Af[k]
            tmp2 = Af[n - k - 1]
            Af[k] = tmp1 + rc * tmp2
            Af[n - k - 1] = tmp2 + rc * tmp1
        Af[n] = rc
        if reached:
            for k in range(n + 1, D):
                Af[k] = 0.0
            stop = n + 1
            break
        for k in range(n + 2):
            tmp1 = CAf[k]
            CAf[k] += rc * CAb[n - k + 1]
            CAb[n - k + 1] += rc * tmp1
    if reached:
        C0 -= _inner(x, x, D)
        nrg_f = C0 * invGain
    else:
        nrg_f = CAf[0]
        tmp1 = 1.0
        for k in range(D):
            Atmp = Af[k]
            nrg_f += CAf[k + 1] * Atmp
            tmp1 += Atmp * Atmp
        nrg_f -= COND_FAC * C0 * tmp1
    A = np.array([F(-a) for a in Af], F)
    if not A.any():
        stop = 0
    return A, F(nrg_f), stop


# -- the reference's tables, built as it builds them -----------------------------

def _tables():
    tw = np.zeros((WINDOW_SIZE, 2), F)
    for i in range(WINDOW_SIZE):
        ph = (-2 * 3.14159265358979323846264338327 / WINDOW_SIZE) * i
        tw[i] = (F(math.cos(ph)), F(math.sin(ph)))
    dct = np.zeros((NB_BANDS, NB_BANDS), F)
    for i in range(NB_BANDS):
        for j in range(NB_BANDS):
            v = F(math.cos((i + .5) * j * math.pi / NB_BANDS))
            if j == 0:
                v = F(float(v) * math.sqrt(.5))
            dct[i, j] = v
    n = np.arange(WINDOW_SIZE)
    d3, r = n // 80, n % 80
    d2, r2 = r // 20, r % 20
    slot = 64 * (r2 % 5) + 16 * (r2 // 5) + 4 * d2 + d3  # kiss_fft's input permutation, factors (4, 4, 4, 5)
    return tw, dct, slot


TW, DCT, SLOT = _tables()
POW995 = [math.pow(.995, i + 1) for i in range(LPC_ORDER)]  # freq.c:174, the libm's


def _cmul(ar, ai, br, bi):
    return ar * br - ai * bi, ar * bi + ai * br


def forward_transform(x: np.ndarray):
    """forward_transform (freq.c:242-254) on the real x [320] float32: opus_fft
    (kiss_fft.c:101-305, 518-586) with the 1/320 scale on the input; returns
    (re, im) of the 320 bins."""
    scale = F(1) / F(320)
    re = np.zeros(WINDOW_SIZE, F)
    im = np.zeros(WINDOW_SIZE, F)
    re[SLOT] = scale * x
    im[SLOT] = scale * np.zeros(WINDOW_SIZE, F)
    twr, twi = TW[:, 0], TW[:, 1]
    # radix 4, m = 1: no twiddles (kiss_fft.c:170-190)
    r, i_ = re.reshape(80, 4), im.reshape(80, 4)
    f0r, f0i, f1r, f1i, f2r, f2i, f3r, f3i = r[:, 0], i_[:, 0], r[:, 1], i_[:, 1], r[:, 2], i_[:, 2], r[:, 3], i_[:, 3]
    s0r, s0i = f0r - f2r, f0i - f2i
    f0r, f0i = f0r + f2r, f0i + f2i
    s1r, s1i = f1r + f3r, f1i + f3i
    o2r, o2i = f0r - s1r, f0i - s1i
    o0r, o0i = f0r + s1r, f0i + s1i
    s1r, s1i = f1r - f3r, f1i - f3i
    re = np.stack([o0r, s0r + s1i, o2r, s0r - s1i], 1).reshape(-1)
    im = np.stack([o0i, s0i - s1r, o2i, s0i + s1r], 1).reshape(-1)
    # radix 4, m = 4 and 16 (kiss_fft.c:191-213)
    for m, ts in ((4, 20), (16, 5)):
        r, i_ = re.reshape(-1, 4, m), im.reshape(-1, 4, m)
        j = np.arange(m)
        ar, ai = _cmul(r[:, 1], i_[:, 1], twr[j * ts], twi[j * ts])
        br, bi = _cmul(r[:, 2], i_[:, 2], twr[2 * j * ts], twi[2 * j * ts])
        cr, ci = _cmul(r[:, 3], i_[:, 3], twr[3 * j * ts], twi[3 * j * ts])
        q0r, q0i = r[:, 0], i_[:, 0]
        dr, di = q0r - br, q0i - bi
        q0r, q0i = q0r + br, q0i + bi
        er, ei = ar + cr, ai + ci
        hr, hi = ar - cr, ai - ci
        re = np.stack([q0r + er, dr + hi, q0r - er, dr - hi], 1).reshape(-1)
        im = np.stack([q0i + ei, di - hr, q0i - ei, di + hr], 1).reshape(-1)
    # radix 5, m = 64 (kiss_fft.c:255-305)
    r, i_ = re.reshape(5, 64), im.reshape(5, 64)
    u = np.arange(64)
    yar, yai, ybr, ybi = twr[64], twi[64], twr[128], twi[128]
    s0r, s0i = r[0], i_[0]
    s1r, s1i = _cmul(r[1], i_[1], twr[u], twi[u])
    s2r, s2i = _cmul(r[2], i_[2], twr[2 * u], twi[2 * u])
    s3r, s3i = _cmul(r[3], i_[3], twr[3 * u], twi[3 * u])
    s4r, s4i = _cmul(r[4], i_[4], twr[4 * u], twi[4 * u])
    s7r, s7i, s10r, s10i = s1r + s4r, s1i + s4i, s1r - s4r, s1i - s4i
    s8r, s8i, s9r, s9i = s2r + s3r, s2i + s3i, s2r - s3r, s2i - s3i
    r0r = s0r + (s7r + s8r)
    r0i = s0i + (s7i + s8i)
    s5r = s0r + ((s7r * yar) + (s8r * ybr))
    s5i = s0i + ((s7i * yar) + (s8i * ybr))
    s6r = (s10i * yai) + (s9i * ybi)
    s6i = -((s10r * yai) + (s9r * ybi))
    s11r = s0r + ((s7r * ybr) + (s8r * yar))
    s11i = s0i + ((s7i * ybr) + (s8i * yar))
    s12r = (s9i * yai) - (s10i * ybi)
    s12i = (s10r * ybi) - (s9r * yai)
    re = np.stack([r0r, s5r - s6r, s11r + s12r, s11r - s12r, s5r + s6r]).reshape(-1)
    im = np.stack([r0i, s5i - s6i, s11i + s12i, s11i - s12i, s5i + s6i]).reshape(-1)
    return re.astype(F), im.astype(F)


def _max16(a, b):
    return a if a > b else b  # arch.h:73


def band_energy_inverse(re: np.ndarray, im: np.ndarray) -> np.ndarray:
    """compute_band_energy_inverse (freq.c:60-84)."""
    tmp = re[:160] * re[:160]
    tmp = tmp + im[:160] * im[:160]  # float32
    inv = (1.0 / (tmp.astype(np.float64) + 1e-9)).astype(F)  # 1.f / (double), rounded to float
    s = [F(0)] * NB_BANDS
    for i in range(NB_BANDS - 1):
        size = (EBAND[i + 1] - EBAND[i]) * 4
        for j in range(size):
            frac = F(j) / F(size)
            t = inv[EBAND[i] * 4 + j]
            s[i] = F(s[i] + F(F(1) - frac) * t)
            s[i + 1] = F(s[i + 1] + frac * t)
    s[0] = F(s[0] * F(2))
    s[-1] = F(s[-1] * F(2))
    return np.array(s, F)


def burg_half(pcm: np.ndarray):
    """compute_burg_cepstrum(pcm, ceps, 80, 16) (freq.c:156-186): (ceps [18],
    A [16], residual energy, stop order)."""
    p = np.asarray(pcm).astype(F)
    assert p.shape == (HALF,)
    burg_in = (p[1:] - PREEMPHASIS * p[:-1]).astype(F)
    A, nrg, stop = silk_burg(burg_in)
    g = F(nrg / F(HALF - 2 * (LPC_ORDER - 1)))
    x = np.zeros(WINDOW_SIZE, F)
    x[0] = 1
    for i in range(LPC_ORDER):
        x[i + 1] = F(float(F(-A[i])) * POW995[i])
    re, im = forward_transform(x)
    E = band_energy_inverse(re, im)
    k = (.45 * float(g)) * float(F(1) / F(F(F(WINDOW_SIZE) * F(WINDOW_SIZE)) * F(WINDOW_SIZE)))
    logMax, follow = F(-2), F(-2)
    Ly = np.zeros(NB_BANDS, F)
    for i in range(NB_BANDS):
        e = F(float(E[i]) * k)
        ly = F(math.log10(1e-2 + float(e)))
        # follow-2.5 is a double difference here (freq.c:180, 182)
        ly = F(_max16(float(F(logMax - F(8))), _max16(float(follow) - 2.5, float(ly))))
        logMax = _max16(logMax, ly)
        follow = F(_max16(float(follow) - 2.5, float(ly)))
        Ly[i] = ly
    ceps = np.zeros(NB_BANDS, F)
    sq = math.sqrt(2. / NB_BANDS)
    for i in range(NB_BANDS):
        acc = F(0)
        for j in range(NB_BANDS):
            acc = F(acc + Ly[j] * DCT[j, i])
        ceps[i] = F(float(acc) * sq)
    ceps[0] = F(ceps[0] + F(-4))
    return ceps, A, nrg, stop


def burg_frame(pcm: np.ndarray):
    """burg_cepstral_analysis (freq.c:188-199) of one frame [160], int16 or
    float32: (ceps [36], A [2, 16], residual energy [2], stop order [2])."""
    p = np.asarray(pcm).astype(F)
    assert p.shape == (FRAME_SIZE,)
    h = [burg_half(p[:HALF]), burg_half(p[HALF:])]
    c0, c1 = h[0][0], h[1][0]
    ceps = np.concatenate([(.5 * (c0 + c1).astype(np.float64)).astype(F), (c0 - c1).astype(F)])
    return ceps, np.stack([h[0][1], h[1][1]]), np.array([h[0][2], h[1][2]], F), np.array([h[0][3], h[1][3]], np.int32)


# -- the compiled reference --------------------------------------------------------

_lib = None


def have_ref() -> bool:
    return O.have_ref()


def ref_lib():
    """oracle/_ref/libref_kernels.so's burg_cepstral_analysis and silk_burg_analysis."""
    global _lib
    if _lib is None:
        l = C.CDLL(O.REF_SO)
        l.burg_cepstral_analysis.argtypes = [C.c_void_p, C.c_void_p]
        l.burg_cepstral_analysis.restype = None
        l.silk_burg_analysis.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int]
        l.silk_burg_analysis.restype = C.c_float
        _lib = l
    return _lib


def ref_frame(pcm: np.ndarray):
    """The compiled reference on one frame: burg_cepstral_analysis, and
    silk_burg_analysis called directly on each half-frame's burg_in; the same
    tuple as burg_frame, stop order from the coefficients."""
    l = ref_lib()
    p = np.ascontiguousarray(np.asarray(pcm).astype(F))
    assert p.shape == (FRAME_SIZE,)
    ceps = np.zeros(2 * NB_BANDS, F)
    l.burg_cepstral_analysis(ceps.ctypes.data, p.ctypes.data)
    A = np.zeros((2, LPC_ORDER), F)
    nrg = np.zeros(2, F)
    for h in range(2):
        q = p[h * HALF:(h + 1) * HALF]
        x = np.ascontiguousarray((q[1:] - PREEMPHASIS * q[:-1]).astype(F))
        nrg[h] = l.silk_burg_analysis(A[h].ctypes.data, x.ctypes.data, C.c_float(1e-3), BURG_LEN, 1, LPC_ORDER)
    return ceps, A, nrg, np.array([stop_from_A(A[0]), stop_from_A(A[1])], np.int32)
