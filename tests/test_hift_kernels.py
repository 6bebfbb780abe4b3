"""Kernel-level tests of the vocoder's element kernels (cosyvoice_amd/csrc/hift_kernels.h) through the narrow entry points cv_hift_source, cv_hift_stft and
cv_hift_istft - the launches of production without the f0 predictor and the convolution stack - at what the whole-model tests on the tiny generator never reach:
more than 512 frames (the second and later chunks of hift_phase_kernel), harmonics that cross the sampling rate (fmodf really wraps), the counter RNG's
distribution, the reflect edges and a second workgroup of the STFT, the exp clip, the output clamp and the withheld tail of the iSTFT.

u = 2^-24 is the unit round-off of fp32 (a correctly rounded operation errs by at most u relative; 1 ulp of a value v is at most 2 u |v|, and at most u for
|v| < 1).  The device's libm functions are charged with the OpenCL full-profile limits (sinf, cosf <= 4 ulp, expf <= 3 ulp, tanhf <= 5 ulp), the host's with 1 ulp.

1. PHASE WALK, bit for bit: phase_out equals a sequential fp32 restatement in numpy (the library is built with -ffp-contract=off, and the product, the division,
   fmod and the sums are all correctly rounded or exact) at 1 .. 1537 frames - four chunks with a one-frame last chunk - on both generators; rows 0 .. 511 of the
   1025-frame run equal the 512-frame run.
2. SOURCE against oracle.hift.sine_gen2 / causal_sine_gen2 + l_linear + tanh on the SAME f0, noise and zero rand_ini.  The oracle's cumsum runs with an fp32
   accumulator (oracle.hift.cumsum_fp32): torch's CPU cumsum accumulates fp32 inputs in double, which is 0.1 rad away from the fp32 value after 1025 frames (the
   error against the unmodified oracle is printed for comparison, not asserted).  The low-rate phase P is then the same fp32 value on both sides and what is left is
      |ds(t)| <= amp uv(t) sum_h |w_h| (k ulp32(max(|P[i0][h]|, |P[i1][h]|)) + e_sin) + e_lin(t) + e_tanh
   with Lipschitz 1 for sin and tanh and
     * k = 3 for the linear up-sampling l0 P[i0] + l1 P[i1] (same l0, l1, i0, i1 on both sides - fp32 formulas of align_corners=False): the device rounds the two
       products and the sum (3 x 1/2 ulp of a value of at most max |P|), the oracle the same three or fewer (an FMA) - 3 ulp together; k = 0 for the causal
       generator's nearest up-sampling (1 P + 0 P is exact);
     * e_sin = 5 u: sinf on the device (4 ulp) and in the oracle (1 ulp), 1 ulp <= u as |sin| <= 1.  The products sin * amp * uv and the sum with the noise term
       are the same operations in the same order on both sides; their roundings are charged to e_lin;
     * e_lin(t) = 2 (H + 4) u (sum_h |wave_h| |w_h| + |b|), |wave_h| <= amp uv + namp |noise|: the roundings of wave_h (two), of the H products with w and of the
       H additions with the bias, on either side, each relative to a partial sum of at most that magnitude;
     * e_tanh = 6 u: tanhf on the device (5 ulp) and tanh in the oracle (1 ulp), |tanh| < 1.
   With voiced f0 <= 150 Hz the bound reaches 5e-3 at the end of 1025 frames (1.6e-6 for the causal generator) against a signal of +-0.2; against the oracle with
   torch's own cumsum the error there is 1.5e-2.  That the bound is not slack: a reference whose P is shifted by ONE frame (P[i + 1] in place of P[i]) violates it on
   most voiced samples (asserted for every case with voiced frames: 93 - 100 % of them).
3. COUNTER RNG: with a one-hot l_linear row (harmonic h), zero bias and f0 = 0 the source is tanh((amp / 3) nz[t][h]), so atanh recovers the draws; moments,
   tail rate, range, independence of harmonics and seeds, reproducibility.  Margins are 5 sigma of the statistic at n = 96 000 draws, not measurements.
4. STFT against torch.stft in float64: per bin |err| <= (16 + c) u S, S = sum_n |x_n w_n|.  16: the roundings of the running sum (15 additions, one product
   x_n tw, each relative to a partial sum of at most S).  c = c_win + c_tw + 1 (the rounding of x_n w_n):
     * the angle a = fl(2 pi_f m) / 16 has relative error <= 1.5 u (pi_f, one rounding), so cosf(a) errs by at most |sin a| a 1.5 u + 4 ulp32(cos a);
     * c_tw: that figure, maximised over the 16 angles (|tw| <= 1, relative to |x_n w_n|);
     * c_win: the window w = 0.5 - 0.5 cosf(a) errs by half that plus u w for the subtraction; relative to w it is largest at n = 1 and 15 (w = 0.038).
   Both constants are evaluated from these formulas (_fp32_constants) and printed; c is about 110, nearly all of it cosf's 4 ulp and the angle's rounding at a = 15 pi / 8 against w = 0.038.
5. SPECTRUM + iSTFT against exp / clip / sin / polar form / torch.istft / clamp in float64 on the same [F][18] input:
      |dy(t)| <= (c_ist + c_chain) u sum_f (V_f / 16) / env(t),   V_f = mag_0 + mag_8 + 2 sum_{k=1..7} mag_k,   f over the (up to 4) frames that contain t
     * c_chain = 15 sqrt(2): |d re|, |d im| <= mag (6 u for expf's 3 ulp - min(., 100) is monotone - + 8 u for sinf(sinf(.)) / cosf(sinf(.)): 4 ulp <= 4 u of the
       inner sine passed on with Lipschitz 1 plus 4 ulp of the outer function, + 1 u for the product), and |c| + |s| <= sqrt(2) for a twiddle pair;
     * c_ist: the twiddle errors (c_tw sqrt(2)), three roundings per bin term, 8 additions per frame, the window's absolute error and the rounding of the product
       with it, 3 additions over the frames, and the relative error of env = sum w^2 (its four terms and three additions, env >= 1.25) with the division,
       applied to |y| <= sum_f (V_f / 16) / env.  Evaluated in _fp32_constants and printed.
   The clamp is 1-Lipschitz, so the same bound holds after it: where the float64 value is within the bound of +-limit either side of the clamp is accepted.

Every operand goes through lib.hook (guard pages under the emulator); outputs carry a sentinel tail that every run checks.  No test runs the convolution stack."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cosyvoice_amd import synthetic as W
from cosyvoice_amd._lib import CosyVoiceAmdError, stream_ptr
from cosyvoice_amd.hift import HiFTGenerator
from oracle import hift as OH

CFG = W.tiny()[2]
H, SCALE, SR = CFG.harmonics + 1, 480, CFG.sr
U, SENTINEL, TAIL = 2.0 ** -24, -6.0e30, 64
K_TRIG, K_EXP, K_TANH, K_HOST = 4, 3, 5, 1            # ulp charged to the device's sinf / cosf, expf, tanhf and to any host function

_p = lambda t: None if t is None else C.c_void_p(t.data_ptr())


def _cfg(causal):
    assert SCALE == CFG.hop * int(np.prod(CFG.ups))
    return dataclasses.replace(CFG, causal=bool(causal))


@functools.lru_cache(maxsize=None)
def _sd(causal):
    return W.make_hift(_cfg(causal))


_handles, _runs = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _drop_handles():
    yield
    _handles.clear()
    _runs.clear()


def _handle(lib, causal, onehot=None):
    """A generator handle on the tiny configuration; onehot = h: l_linear picks harmonic h alone, zero bias."""
    key = (id(lib), bool(causal), onehot)
    if key not in _handles:
        sd = dict(_sd(bool(causal)))
        if onehot is not None:
            sd["m_source.l_linear.weight"] = F.one_hot(torch.tensor([onehot]), H).float()
            sd["m_source.l_linear.bias"] = torch.zeros(1)
        _handles[key] = HiFTGenerator(sd, _cfg(causal), lib=lib)
    return _handles[key]


def _source(lib, causal, f0, noise=None, seed=0, onehot=None):
    """cv_hift_source -> (P [m][H] numpy fp32, s [480 m] torch fp32); the sentinel tails of both outputs are checked."""
    m = int(f0.numel())
    L = m * SCALE
    h = _handle(lib, causal, onehot)
    f0d = lib.hook(f0.to(lib.device, torch.float32).contiguous())
    nz = None if noise is None else lib.hook(noise.to(lib.device, torch.float32).reshape(L, H).contiguous())
    P = lib.hook(torch.full((m + 1, H), SENTINEL, device=lib.device))
    s = lib.hook(torch.full((L + TAIL,), SENTINEL, device=lib.device))
    lib.cv_hift_source(h._h, _p(f0d), C.c_int32(m), _p(nz), C.c_uint64(seed), _p(P), _p(s), stream_ptr(lib))
    if not lib.emulated:
        torch.cuda.current_stream().synchronize()
    P, s = P.cpu(), s.cpu()
    assert bool((P[m] == SENTINEL).all()) and bool((s[L:] == SENTINEL).all()), "written outside the valid outputs"
    assert bool(torch.isfinite(P[:m]).all()) and bool((P[:m] != SENTINEL).all()) and bool((s[:L].abs() <= 1).all()), "a valid output was not written"
    return P[:m].numpy().copy(), s[:L].clone()


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. phase walk
# ------------------------------------------------------------------------------------------------------------------------------------
def _phase_restatement(f0):
    """hift_phase_kernel in sequential fp32: -> (P [m][H], q = fn / sr [m][H]), every operation one correctly rounded fp32 operation."""
    f0 = np.asarray(f0, np.float32)
    fn = f0[:, None] * np.arange(1, H + 1, dtype=np.float32)[None]
    q = fn / np.float32(SR)
    rad = np.fmod(q, np.float32(1))
    assert fn.dtype == q.dtype == rad.dtype == np.float32
    P, c = np.empty((f0.size, H), np.float32), np.zeros(H, np.float32)
    for i in range(f0.size):
        c = c + rad[i]
        P[i] = ((c * np.float32(2)) * np.float32(np.pi)) * np.float32(SCALE)
    assert P.dtype == np.float32
    return P, q


WALK_FRAMES = (1, 2, 511, 512, 513, 1024, 1025, 1537)


@functools.lru_cache(maxsize=None)
def _f0_walk():
    """1537 seeded frames in stretches of 3 .. 40: voiced 60 - 400 Hz, exact zeros, 2700 - 3100 Hz (harmonics 8 and 9 cross sr = 24 kHz); frame 0 is 3050 Hz, frame 1 is 0,
    and a high stretch lies across the first chunk boundary (frames 508 .. 515).  Every frame count of the test takes the leading frames."""
    rng = np.random.default_rng(512)
    f0, kind, i, k = np.zeros(1537, np.float32), np.zeros(1537, np.int8), 2, 0
    while i < 1537:
        n = int(rng.integers(3, 41))
        if k % 3 == 0:
            f0[i:i + n] = rng.uniform(60, 400, n)[:f0[i:i + n].size]
        elif k % 3 == 2:
            f0[i:i + n] = rng.uniform(2700, 3100, n)[:f0[i:i + n].size]
        kind[i:i + n] = k % 3
        i, k = i + n, k + 1
    f0[0], kind[0], f0[1], kind[1] = 3050.0, 2, 0.0, 1
    f0[508:516], kind[508:516] = rng.uniform(2700, 3100, 8), 2
    assert all((kind == j).sum() > 300 for j in range(3))
    return torch.from_numpy(f0), kind


def _walk(lib, causal, m):
    key = (id(lib), "walk", bool(causal), m)
    if key not in _runs:
        _runs[key] = _source(lib, causal, _f0_walk()[0][:m], seed=7)[0]
    return _runs[key]


@pytest.mark.parametrize("causal", [False, True], ids=["hift", "causal"])
def test_phase_walk_equals_the_sequential_fp32_sum_bit_for_bit(lib, causal):
    """Bit-identical on the emulator and on the MI355X (fp32 multiply, divide, fmod and add are correctly rounded or exact on both)."""
    f0, kind = _f0_walk()
    ref, q = _phase_restatement(f0.numpy())
    hi = kind == 2
    assert bool((q[hi][:, 8] >= 1).all()) and bool((q[hi][:, 7] >= 1).any()) and bool((q[hi][:, :7] < 1).all())     # harmonics 8 and 9 wrap, and only they
    assert bool((q[~hi] < 1).all()) and bool((ref[kind == 1][:, 0] == ref[np.flatnonzero(kind == 1) - 1][:, 0]).all())   # f0 = 0 adds nothing
    for m in WALK_FRAMES:
        got = _walk(lib, causal, m)
        same = got.view(np.uint32) == ref[:m].view(np.uint32)
        assert same.all(), (m, int((~same).sum()), np.argwhere(~same)[:4].tolist(), float(np.abs(got.astype(np.float64) - ref[:m]).max()))
    assert np.array_equal(_walk(lib, causal, 1025)[:512].view(np.uint32), _walk(lib, causal, 512).view(np.uint32))      # prefix: nothing leaks back over a chunk boundary


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. source
# ------------------------------------------------------------------------------------------------------------------------------------
def _f0_mixed(m, seed):
    """Voiced stretches of 60 - 150 Hz and unvoiced ones (f0 = 0 or 5 Hz, below voiced_thr), 1 .. 30 frames each."""
    rng = np.random.default_rng(seed)
    f0, i, k = np.zeros(m, np.float32), 0, 0
    while i < m:
        n = int(rng.integers(1, 31))
        f0[i:i + n] = (rng.uniform(60, 150, n) if k % 2 == 0 else np.full(n, 5.0 * (k % 4 == 1)))[:f0[i:i + n].size]
        i, k = i + n, k + 1
    return torch.from_numpy(f0)


THR = np.float32(CFG.voiced_thr)
#               name: (f0, noise scale, shifted-reference check)
SOURCE_CASES = {
    "m3-noise": (lambda: torch.tensor([0.0, 120.0, 95.0]), 1.0, True),                                # first / last frame: src clamps to 0, i1 clamps to m - 1
    "m513-noise": (lambda: _f0_mixed(513, 1), 1.0, True),                                             # one frame into the second chunk
    "m1025": (lambda: _f0_mixed(1025, 2), 0.0, True),                                                 # one frame into the third chunk, zero noise
    "thr": (lambda: torch.from_numpy(np.array([THR, np.nextafter(THR, np.float32(20)), THR, np.nextafter(THR, np.float32(20)), THR], np.float32)), 1.0, True),
    "unvoiced": (lambda: torch.tensor([0.0, 9.5, 0.0, 3.0]), 1.0, False),
    "voiced": (lambda: torch.tensor([100.0, 150.0, 61.5, 149.0, 88.0, 131.0, 75.0]), 1.0, True),
}


def _interp_indices(m, causal):
    """i0, i1, l0, l1 of hift_source_kernel (= torch's linear up-sampling with align_corners=False, or nearest for the causal generator), in fp32."""
    t = np.arange(m * SCALE)
    if causal:
        i0 = t // SCALE
        return i0, i0, np.ones(t.size, np.float32), np.zeros(t.size, np.float32)
    src = np.maximum(np.float32(1.0 / SCALE) * (t.astype(np.float32) + np.float32(0.5)) - np.float32(0.5), np.float32(0))
    i0 = src.astype(np.int64)
    i1 = i0 + (i0 < m - 1)
    l1 = src - i0.astype(np.float32)
    return i0, i1, np.float32(1) - l1, l1


@functools.lru_cache(maxsize=None)
def _source_case(name, causal):
    """Inputs, the oracle's source (fp32 cumsum; and with torch's own cumsum, for the printed comparison), the per-sample bound and the shifted reference."""
    make_f0, nscale, shift = SOURCE_CASES[name]
    cfg, sd = _cfg(causal), _sd(causal)
    f0 = make_f0()
    m = f0.numel()
    L = m * SCALE
    g = torch.Generator().manual_seed(100 + m)
    noise = (torch.rand(L, H, generator=g) if causal else torch.randn(L, H, generator=g)) * nscale          # the causal generator's noise is uniform
    w, b = sd["m_source.l_linear.weight"], sd["m_source.l_linear.bias"]
    f0_up = F.interpolate(f0[None, None], scale_factor=float(SCALE), mode="nearest").transpose(1, 2)        # what HiFTGenerator.inference feeds SineGen2
    gen = (lambda c: OH.causal_sine_gen2(cfg, f0_up, torch.zeros(1, H), noise[None], cumsum=c)) if causal else \
          (lambda c: OH.sine_gen2(cfg, f0_up, torch.zeros(1, H), noise[None], cumsum=c)[0])
    want = torch.tanh(F.linear(gen(OH.cumsum_fp32), w, b))[0, :, 0]
    want_f64acc = torch.tanh(F.linear(gen(torch.cumsum), w, b))[0, :, 0]
    # bound
    P = _phase_restatement(f0.numpy())[0]
    i0, i1, l0, l1 = _interp_indices(m, causal)
    aw, amp = w[0].abs().double().numpy(), cfg.nsf_alpha
    uv = (f0.numpy() > THR).astype(np.float64)[np.arange(L) // SCALE]
    namp = uv * cfg.nsf_sigma + (1 - uv) * amp / 3
    ulp = np.spacing(np.maximum(np.abs(P[i0]), np.abs(P[i1]))).astype(np.float64)
    k = 0 if causal else 3
    e_lin = 2 * (H + 4) * U * (((amp * uv)[:, None] + namp[:, None] * noise.abs().double().numpy()) @ aw + abs(float(b)))
    bound = amp * uv * ((k * ulp + (K_TRIG + K_HOST) * U) @ aw) + e_lin + (K_TANH + K_HOST) * U
    # the same reference with the phase of frame i + 1 in place of frame i (the last frame extrapolated), restated in float64 on the fp32 P
    shifted = None
    if shift:
        Ps = np.concatenate([P[1:], P[-1:] + (P[-1:] - P[-2:-1])]).astype(np.float64)
        ph = l0.astype(np.float64)[:, None] * Ps[i0] + l1.astype(np.float64)[:, None] * Ps[i1]
        wave = np.sin(ph) * amp * uv[:, None] + namp[:, None] * noise.double().numpy()
        shifted = np.tanh(wave @ w[0].double().numpy() + float(b))
    return dict(f0=f0, noise=noise, want=want.double().numpy(), want_f64acc=want_f64acc.double().numpy(), bound=bound, uv=uv, shifted=shifted)


@pytest.mark.parametrize("causal", [False, True], ids=["hift", "causal"])
@pytest.mark.parametrize("name", list(SOURCE_CASES))
def test_source_against_the_oracle_on_the_same_f0(lib, name, causal):
    c = _source_case(name, causal)
    P, s = _source(lib, causal, c["f0"], noise=c["noise"])
    assert np.array_equal(P.view(np.uint32), _phase_restatement(c["f0"].numpy())[0].view(np.uint32))
    err = np.abs(s.double().numpy() - c["want"])
    ratio = err / c["bound"]
    print("hift_source_kernel %s %s: worst |err| / bound = %.3g (max |err| %.3g, max bound %.3g; against torch's double-accumulating cumsum: max |err| %.3g)"
          % (name, "causal" if causal else "hift", ratio.max(), err.max(), c["bound"].max(), np.abs(s.double().numpy() - c["want_f64acc"]).max()))
    assert ratio[0] <= 1 and bool((ratio[-SCALE:] <= 1).all()), "sample 0 (src clamps to 0) / the last frame (i1 clamps)"
    assert bool((err <= c["bound"]).all()), (float(ratio.max()), int(ratio.argmax()))
    voiced = c["uv"] > 0
    if name == "unvoiced":
        assert not voiced.any()
    if name == "thr":                                        # f0 == voiced_thr is unvoiced (f0 > thr), one ulp above is voiced
        assert np.array_equal(voiced[::SCALE], np.array([False, True, False, True, False]))
    if c["shifted"] is not None:                             # the bound is not slack: one frame of phase shift breaks it on most voiced samples
        broken = (np.abs(c["shifted"] - c["want"]) > c["bound"])[voiced].mean()
        print("    reference with P shifted by one frame: outside the bound on %.1f %% of the voiced samples" % (100 * broken))
        assert voiced.any() and broken > 0.5, broken


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. counter RNG
# ------------------------------------------------------------------------------------------------------------------------------------
RNG_FRAMES = 200
N_DRAWS = RNG_FRAMES * SCALE


def _draws(lib, causal, h, seed, fresh=False):
    """The n = 96 000 draws of harmonic h under `seed`, recovered from s = tanh((amp / 3) nz) (float64), and the raw source."""
    key = (id(lib), "rng", bool(causal), h, seed)
    if fresh or key not in _runs:
        s = _source(lib, causal, torch.zeros(RNG_FRAMES), noise=None, seed=seed, onehot=h)[1]
        namp = np.float32(np.float32(np.float32(1) * np.float32(CFG.nsf_alpha)) / np.float32(3))
        run = (np.arctanh(s.double().numpy()) / float(namp), s)
        if fresh:
            return run
        _runs[key] = run
    return _runs[key]


def _corr(a, b):
    return float(np.corrcoef(a, b)[0, 1])


@pytest.mark.parametrize("h", [0, 4, 8])
def test_counter_rng_gaussian_draws_of_the_non_causal_source(lib, h):
    n = N_DRAWS
    x, _ = _draws(lib, False, h, 1986)
    assert x.size == n and abs(x.mean()) < 5 / np.sqrt(n), x.mean()
    assert abs(x.var() - 1) < 5 * np.sqrt(2 / n), x.var()
    p = 2.6998e-3                                            # P(|N(0, 1)| > 3)
    assert abs((np.abs(x) > 3).mean() - p) < 5 * np.sqrt(p * (1 - p) / n), (np.abs(x) > 3).mean()


@pytest.mark.parametrize("h", [0, 4, 8])
def test_counter_rng_uniform_draws_of_the_causal_source(lib, h):
    n = N_DRAWS
    x, s = _draws(lib, True, h, 1986)
    assert x.size == n and float(s.min()) >= 0 and x.min() >= 0 and x.max() < 1, (x.min(), x.max())
    assert abs(x.mean() - 0.5) < 5 / np.sqrt(12 * n), x.mean()
    assert abs(x.var() - 1 / 12) < 5 * np.sqrt((1 / 80 - 1 / 144) / n), x.var()      # var of the sample variance = (mu_4 - sigma^4) / n


@pytest.mark.parametrize("causal", [False, True], ids=["hift", "causal"])
def test_counter_rng_streams_are_independent_and_reproducible(lib, causal):
    lim = 5 / np.sqrt(N_DRAWS)
    x = {h: _draws(lib, causal, h, 1986)[0] for h in (0, 4, 8)}
    for a, b in ((0, 4), (4, 8), (0, 8)):
        assert abs(_corr(x[a], x[b])) < lim, (a, b, _corr(x[a], x[b]))
    other = _draws(lib, causal, 4, 1987)[0]
    assert abs(_corr(x[4], other)) < lim, _corr(x[4], other)
    assert abs(_corr(x[4][1:], x[4][:-1])) < lim and abs(_corr(x[4][SCALE:], x[4][:-SCALE])) < lim            # no lag-1 / lag-one-frame structure either
    again = _draws(lib, causal, 4, 1986, fresh=True)[1]
    assert torch.equal(again, _draws(lib, causal, 4, 1986)[1])                                                   # same seed, same bits


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. / 5. STFT, spectrum + iSTFT
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fp32_constants():
    """The error constants of the docstring, in units of u, from the stated charges."""
    a = 2 * np.pi * np.arange(16) / 16
    ulp_cos = np.spacing(np.abs(np.cos(a)).astype(np.float32)).astype(np.float64) / U         # 1 ulp of |cos a| in units of u (at most 1)
    ulp_sin = np.spacing(np.abs(np.sin(a)).astype(np.float32)).astype(np.float64) / U
    d_cos = np.abs(np.sin(a)) * a * 1.5 + K_TRIG * ulp_cos                                     # absolute error of cosf(a) / sinf(a) on the device
    d_sin = np.abs(np.cos(a)) * a * 1.5 + K_TRIG * ulp_sin
    c_tw = float(max(d_cos.max(), d_sin.max()))
    w = 0.5 - 0.5 * np.cos(a)
    d_win = 0.5 * d_cos + w                                                                    # absolute error of the device's window
    c_win = float((d_win[1:] / w[1:]).max())                                                   # w_0 = 0.5 - 0.5 cosf(0) = 0 exactly
    c_stft = c_win + c_tw + 1
    dw = float(d_win.max())
    sq2 = np.sqrt(2.0)
    c_chain = (2 * K_EXP + 2 * K_TRIG + 1) * sq2
    c_frame = (c_tw * sq2 + 3 + 8) + dw + 1                  # bin terms: twiddles, 2 products + 1 subtraction; 8 additions; the window's error; the product with it
    c_env = ((4 * (2 * dw + 1) + 3 * 1.5) / 1.25) + 1         # four w^2 terms, three additions of at most env <= 1.5, over env >= 1.25; the division
    return dict(c_stft=c_stft, c_win=c_win, c_tw=c_tw, c_ist=c_frame + 3 + c_env, c_chain=c_chain)


def _hann64():
    n = torch.arange(16, dtype=torch.float64)
    return 0.5 - 0.5 * torch.cos(2 * np.pi * n / 16)


def _stft_input(kind, L):
    if kind == "impulses":
        x = torch.zeros(L)
        x[0], x[1], x[L - 2], x[L - 1] = 1.0, -1.0, -1.0, 1.0
        return x
    return torch.tanh(torch.randn(L, generator=torch.Generator().manual_seed(L)))


@pytest.mark.parametrize("kind,L", [("tanh", 16), ("tanh", 480), ("tanh", 1440), ("tanh", 1028), ("impulses", 16), ("impulses", 1028)])
def test_stft_against_float64(lib, kind, L):
    x = _stft_input(kind, L)
    Fr = L // 4 + 1
    xd = lib.hook(x.to(lib.device))
    out = lib.hook(torch.full((Fr + 1, 18), SENTINEL, device=lib.device))
    lib.cv_hift_stft(_p(xd), C.c_int64(L), _p(out), stream_ptr(lib))
    if not lib.emulated:
        torch.cuda.current_stream().synchronize()
    out = out.cpu()
    assert bool((out[Fr] == SENTINEL).all()) and bool((out[:Fr] != SENTINEL).all())
    win = _hann64()
    ref = torch.stft(x.double(), 16, 4, 16, window=win, center=True, pad_mode="reflect", return_complex=True)           # [9][F]
    assert ref.shape == (9, Fr)
    want = torch.cat([ref.real.T, ref.imag.T], dim=1)                                                                      # [F][re(9) | im(9)]
    frames = F.pad(x.double()[None, None], (8, 8), mode="reflect")[0, 0].unfold(0, 16, 4)                                  # [F][16]
    S = (frames.abs() * win).sum(1, keepdim=True)
    k = _fp32_constants()
    bound = (16 + k["c_stft"]) * U * S
    err = (out[:Fr].double() - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print("hift_stft_kernel %s L=%d: worst |err| / bound = %.3g  (c = %.1f: window %.1f + twiddles %.1f + 1)" % (kind, L, ratio, k["c_stft"], k["c_win"], k["c_tw"]))
    assert bool((err <= bound).all()), ratio


ISTFT_SEED = 1       # chosen on the CPU: the float64 reference clamps 37 - 41 % of the samples at every F below - non-zero and below one half (asserted in the test)


@functools.lru_cache(maxsize=None)
def _istft_case(Fr):
    """conv_post-like input [F][18]: log-magnitudes randn * 1.5 with one row in sixteen lifted above ln 100 (the clip is active), phases randn * 4; the float64
    restatement before the clamp and the per-sample bound, both for the full length 4 (F - 1)."""
    g = torch.Generator().manual_seed(ISTFT_SEED)
    x = torch.cat([torch.randn(Fr, 9, generator=g) * 1.5, torch.randn(Fr, 9, generator=g) * 4], dim=1)
    x[::16, :9] = x[::16, :9].abs() + 4.7
    xd = x.double()
    raw = torch.exp(xd[:, :9])
    mag, ph = torch.clip(raw, max=100.0), torch.sin(xd[:, 9:])
    assert bool((raw[::16] > 100).all()) and bool((raw < 100).any())
    y = torch.istft(torch.complex(mag * torch.cos(ph), mag * torch.sin(ph)).T[None], 16, 4, 16, window=_hann64())[0]
    L = 4 * (Fr - 1)
    assert y.shape == (L,)
    V = (mag[:, 0] + mag[:, 8] + 2 * mag[:, 1:8].sum(1)) / 16
    win2 = _hann64() ** 2
    sumV, env = torch.zeros(L, dtype=torch.float64), torch.zeros(L, dtype=torch.float64)
    tp = torch.arange(L) + 8
    for j in range(4):
        f = tp // 4 - j
        ok = (f >= 0) & (f < Fr)
        n = (tp - 4 * f).clamp(0, 15)
        sumV += torch.where(ok, V[f.clamp(0, Fr - 1)], torch.zeros(()).double())
        env += torch.where(ok, win2[n], torch.zeros(()).double())
    assert float(env.min()) >= 1.25 - 1e-12 and float(env.max()) <= 1.5 + 1e-12
    k = _fp32_constants()
    return x, y, (k["c_ist"] + k["c_chain"]) * U * sumV / env


@pytest.mark.parametrize("Fr,cut", [(5, 0), (121, 0), (258, 0), (361, 0), (361, 480)], ids=["F5", "F121", "F258", "F361", "F361-withheld-480"])
def test_spectrum_and_istft_against_float64(lib, Fr, cut):
    x, y, bound = _istft_case(Fr)
    L, limit = 4 * (Fr - 1) - cut, CFG.audio_limit
    want, bound = y[:L].clamp(-limit, limit), bound[:L]
    share = float((y[:L].abs() >= limit).double().mean())
    assert 0 < share < 0.5, share                                                                      # the clamp is active, and not everywhere
    spec = lib.hook(x.to(lib.device).clone())
    out = lib.hook(torch.full((L + TAIL,), SENTINEL, device=lib.device))
    lib.cv_hift_istft(_p(spec), C.c_int64(Fr), C.c_int64(L), C.c_float(limit), _p(out), stream_ptr(lib))
    if not lib.emulated:
        torch.cuda.current_stream().synchronize()
    out = out.cpu()
    assert bool((out[L:] == SENTINEL).all()) and bool((out[:L].abs() <= np.float32(limit)).all())
    err = (out[:L].double() - want).abs()
    ratio = float((err / bound).max())
    k = _fp32_constants()
    print("hift_spec_kernel + hift_istft_kernel F=%d L=%d: worst |err| / bound = %.3g, clamped share %.3f  (c_ist = %.1f, c_chain = %.1f)"
          % (Fr, L, ratio, share, k["c_ist"], k["c_chain"]))
    assert bool((err <= bound).all()), ratio
    assert bool((out[:L][(y[:L].abs() - limit) > bound] .abs() == np.float32(limit)).all())            # clearly beyond the limit: exactly +-limit


# ------------------------------------------------------------------------------------------------------------------------------------
# argument checks: an error return, not a launch (emulator only)
# ------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments(emu_lib):
    lib = emu_lib
    h = _handle(lib, False)
    f0, P, s = lib.hook(torch.zeros(4)), lib.hook(torch.zeros(4, H)), lib.hook(torch.zeros(4 * SCALE))
    src = lambda *a: lib.cv_hift_source(a[0], a[1], C.c_int32(a[2]), None, C.c_uint64(0), a[3], a[4], None)
    for args in ((None, _p(f0), 4, _p(P), _p(s)), (h._h, None, 4, _p(P), _p(s)), (h._h, _p(f0), 4, _p(P), None), (h._h, _p(f0), 0, _p(P), _p(s)), (h._h, _p(f0), -3, _p(P), _p(s))):
        with pytest.raises(CosyVoiceAmdError, match="cv_hift_source"):
            src(*args)
    src(h._h, _p(f0), 4, None, _p(s))                                                                  # phase_out is optional
    x, o = lib.hook(torch.zeros(32)), lib.hook(torch.zeros(9, 18))
    for a, L, b in ((None, 32, _p(o)), (_p(x), 32, None), (_p(x), 12, _p(o)), (_p(x), 18, _p(o)), (_p(x), 0, _p(o)), (_p(x), -16, _p(o))):
        with pytest.raises(CosyVoiceAmdError, match="cv_hift_stft"):
            lib.cv_hift_stft(a, C.c_int64(L), b, None)
    sp, y = lib.hook(torch.zeros(9, 18)), lib.hook(torch.zeros(32))
    for a, Fr, L, lim, b in ((None, 9, 32, 0.99, _p(y)), (_p(sp), 9, 32, 0.99, None), (_p(sp), 9, 36, 0.99, _p(y)), (_p(sp), 1, 0, 0.99, _p(y)), (_p(sp), 9, 0, 0.99, _p(y)),
                             (_p(sp), 9, 32, 0.0, _p(y)), (_p(sp), 9, 32, float("nan"), _p(y))):
        with pytest.raises(CosyVoiceAmdError, match="cv_hift_istft"):
            lib.cv_hift_istft(a, C.c_int64(Fr), C.c_int64(L), C.c_float(lim), b, None)
