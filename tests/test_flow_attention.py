"""The flow estimator's bf16 flash attention (attn_flow32_kernel, csrc/flow_attn32.h) against a float64 reference, through its test entry point
cv_flow_attention_bf16 - the production grid, workgroup remap and instantiations of every bf16 estimator pass.

Reference: the fp32 operands are rounded to bf16 first (those are the kernel's exact operands); S = scale q.k^T, the mask, the softmax and P.V are float64.
V^T is packed with a restatement of the layout contract (inside every 32-key block, key 16 s + 4 g + r sits at column 8 g + 4 s + r), not with the library's
vt_col.  Every operand is allocated at its exact size through lib.hook: under the emulator it ends flush against an inaccessible page.

Tolerance (derived, not tuned).  The bf16 products are exact and S is accumulated in fp32 (relative error ~2^-24 per term: negligible next to what follows).
P is rounded to bf16 before P.V, relative error <= 2^-8 per probability, while the denominator sums the unrounded P: the numerator is off by at most
2^-8 sum_j p_j |v_j| / sum_j p_j <= 2^-8 max|v over the visible keys|.  The output is rounded to bf16: another 2^-8 |o|.  So per element
    |o - ref| <= 2^-8 (vmax + |ref|) (1 + EPS),
EPS = 2^-5 for the fp32 score / exp2 / denominator rounding.  A query that sees one key too many or too few, a wrong key order or a wrong rescale breaks
this by orders of magnitude with the inputs below (dominant keys, distinctive V), not by a bf16-sized amount.  The mean error is bounded too:
mean|o - ref| <= MEAN_BOUND mean(vmax), MEAN_BOUND calibrated once: the largest ratio over the cases below is 2.6e-4 (the lazy-rescale case), ~2.3x margin.

Emulator share of this file: about 10 s on one worker (the T = 674 / 1348 cases run on the hardware only)."""
import ctypes as C

import pytest
import torch

from cosyvoice_amd._lib import CosyVoiceAmdError, stream_ptr

SCALE = 0.125                     # the estimator's 1 / sqrt(64)
EPS = 2.0 ** -5
MEAN_BOUND = 6e-4
SENTINEL = -8531                  # int16 bits of bf16 0xdead (-6.2e18): what an unwritten output element holds
THR_LOG2 = 8.0                    # the kernel's lazy-rescale threshold in log2 units (flow_attn32.h: THR)


def _sync(lib):
    if not lib.emulated:
        torch.cuda.synchronize()


def _bf(x):
    return x.to(torch.bfloat16).float()


def _vt_cols(T):
    t = torch.arange(T)
    return 32 * (t // 32) + 8 * ((t // 4) % 4) + 4 * ((t // 16) % 2) + t % 4


def _round_up(x, m):
    return (x + m - 1) // m * m


class Run:
    """One launch of the kernel: output bits [B * T + extra_rows][ldo] as int16 and the values of the problem's part as float [B, T, H, 64]."""

    def __init__(self, bits, B, T, H):
        self.bits = bits
        self.o = bits[:B * T, :64 * H].view(torch.bfloat16).float().reshape(B, T, H, 64)


def _launch(lib, q, k, v, *, chunk=0, klen=None, waves=0, interleave=False, ldt=None, ldo=None, extra_rows=0, vt_pad=0.0):
    """q, k, v: bf16-exact float [B, T, H, 64].  interleave: q and k share one [B T][128 H] buffer as the estimator's QKV epilogue writes them (k at column 64 H);
    vt_pad: the value of every V^T column that holds no key (columns of keys >= T, up to ldt)."""
    B, T, H, _ = q.shape
    dev = lib.device
    HD = 64 * H
    if interleave:
        ld = 2 * HD
        qk = torch.cat([q.reshape(B * T, HD), k.reshape(B * T, HD)], 1).to(torch.bfloat16)
        qk = lib.hook(qk.to(dev))
        keep = [qk]
        qp, kp = qk.data_ptr(), qk.data_ptr() + 2 * HD
    else:
        ld = HD
        qt = lib.hook(q.reshape(B * T, HD).to(torch.bfloat16).to(dev)); kt = lib.hook(k.reshape(B * T, HD).to(torch.bfloat16).to(dev))
        keep = [qt, kt]
        qp, kp = qt.data_ptr(), kt.data_ptr()
    ldt = ldt or _round_up(T, 64)
    vt = torch.full((B, HD, ldt), vt_pad, dtype=torch.float32)
    vt[:, :, _vt_cols(T)] = v.reshape(B, T, HD).transpose(1, 2)
    vt = lib.hook(vt.to(torch.bfloat16).to(dev))
    ldo = ldo or HD
    o = lib.hook(torch.full((B * T + extra_rows, ldo), SENTINEL, dtype=torch.int16).view(torch.bfloat16).to(dev))
    kl = lib.hook(torch.tensor(klen, dtype=torch.int32).to(dev)) if klen is not None else None
    keep += [vt, o, kl]
    lib.cv_flow_attention_bf16(C.c_void_p(qp), C.c_void_p(kp), C.c_int32(ld), C.c_void_p(vt.data_ptr()), C.c_int64(HD * ldt), C.c_int32(ldt),
                               C.c_void_p(o.data_ptr()), C.c_int32(ldo), C.c_int32(B), C.c_int32(H), C.c_int32(T), C.c_float(SCALE), C.c_int32(chunk),
                               C.c_void_p(kl.data_ptr() if kl is not None else None), C.c_int32(waves), stream_ptr(lib))
    _sync(lib)
    return Run(o.cpu().view(torch.int16).clone(), B, T, H)


def _visible(T, n, chunk):
    """[T queries, T keys] bool: key j visible to query i in a batch row with n keys."""
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    vis = j < n
    if chunk > 0:
        vis = vis & (j < (i // chunk + 1) * chunk)
    return vis


def _reference(q, k, v, chunk=0, klen=None):
    """float64 attention of the bf16 operands -> (out [B, T, H, 64], vmax [B, T, H] = max |v| over the keys a query sees)."""
    B, T, H, _ = q.shape
    out = torch.zeros(B, T, H, 64, dtype=torch.float64)
    vmax = torch.zeros(B, T, H, dtype=torch.float64)
    for b in range(B):
        n = T if klen is None else min(T, klen[b])
        vis = _visible(T, n, chunk)
        qd, kd, vd = q[b].double(), k[b].double(), v[b].double()
        s = torch.einsum("qhd,khd->hqk", qd, kd) * SCALE
        s = s.masked_fill(~vis[None], float("-inf"))
        p = torch.softmax(s, -1).nan_to_num(0.0)                 # a query without keys: all-zero output (the kernel's l > 0 guard)
        out[b] = torch.einsum("hqk,khd->qhd", p, vd)
        va = vd.abs().amax(-1)                                   # [keys, H]
        vmax[b] = torch.where(vis[:, :, None], va[None], torch.zeros(())).amax(1)
    return out, vmax


def _check(run, q, k, v, chunk=0, klen=None, what=""):
    ref, vmax = _reference(q, k, v, chunk, klen)
    err = (run.o.double() - ref).abs()
    bound = 2.0 ** -8 * (vmax[..., None] + ref.abs()) * (1 + EPS)
    worst = (err - bound).flatten().argmax().item()
    assert bool((err <= bound).all()), ("%s: |o - ref| above the bf16 bound at flat index %d: err %.4g, bound %.4g, ref %.4g, o %.4g"
                                        % (what, worst, err.flatten()[worst].item(), bound.flatten()[worst].item(), ref.flatten()[worst].item(), run.o.flatten()[worst].item()))
    mean_ratio = err.mean().item() / max(vmax.mean().item(), 1e-30)
    assert mean_ratio <= MEAN_BOUND, (what, mean_ratio)
    return ref


def _randn(shape, seed, std=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * std


def _random_case(B, T, H, seed):
    q = _bf(_randn((B, T, H, 64), seed)); k = _bf(_randn((B, T, H, 64), seed + 1)); v = _bf(_randn((B, T, H, 64), seed + 2))
    return q, k, v


def _assert_untouched(run, B, T, H):
    """Every output element of the problem written; pad columns (ldo > 64 H) and rows past B T hold the sentinel."""
    assert not bool((run.bits[:B * T, :64 * H] == SENTINEL).any()), "an output element of the problem was not written"
    assert bool((run.bits[:B * T, 64 * H:] == SENTINEL).all()), "a write into the pad columns of o"
    assert bool((run.bits[B * T:] == SENTINEL).all()), "a write past row B T of o"


# ---- shapes ----------------------------------------------------------------------------------------------------------------------------------------------

_TS = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193]
_BH = [(1, 1), (3, 2), (1, 2), (3, 1)]


@pytest.mark.parametrize("T", _TS)
def test_shapes_against_fp64(lib, T):
    """T over 1 .. 193: partial query tiles of 32 / 64 / 128, partial last key tile (rows >= T clamped to T - 1 and masked), every ntile % 3 of the 3-stage ring
    (1 .. 4 key tiles).  B x H cycles over 1 x 1, 3 x 2, 1 x 2, 3 x 1.  Both workgroup shapes (2 and 4 waves) must give the same bits (the header contract of
    flow_attn32.h); o has pad columns and a spare row that must keep the sentinel; with B = 3 the middle batch row must equal its own B = 1 launch bit for bit."""
    B, H = _BH[_TS.index(T) % len(_BH)]
    q, k, v = _random_case(B, T, H, 100 + T)
    r2 = _launch(lib, q, k, v, waves=2, ldo=64 * H + 4, extra_rows=1)
    r4 = _launch(lib, q, k, v, waves=4, ldo=64 * H + 4, extra_rows=1)
    _assert_untouched(r2, B, T, H); _assert_untouched(r4, B, T, H)
    assert torch.equal(r2.bits, r4.bits), "2 and 4 waves per workgroup differ"
    _check(r4, q, k, v, what="T=%d B=%d H=%d" % (T, B, H))
    r0 = _launch(lib, q, k, v)                                   # waves = 0: the estimator's default (4)
    assert torch.equal(r0.bits, r4.bits[:B * T, :64 * H])
    if B == 3:
        alone = _launch(lib, q[1:2], k[1:2], v[1:2])
        assert torch.equal(alone.bits, r4.bits[T:2 * T, :64 * H]), "a batch row depends on the other rows of its launch"


@pytest.mark.parametrize("chunk", [0, 50])
def test_estimator_geometry(lib, chunk):
    """q and k interleaved in one [B T][128 H] buffer (k at column 64 H: attn_flow's operands), V^T with ldt larger than T rounded up to 64 and a pad
    region of large finite values (the precondition: finite, never weighted), the estimator's chunk of 50 and none."""
    B, T, H = 2, 150, 2
    q, k, v = _random_case(B, T, H, 7)
    run = _launch(lib, q, k, v, chunk=chunk, interleave=True, ldt=_round_up(T, 64) + 64, vt_pad=3.0e4)
    _check(run, q, k, v, chunk, what="estimator geometry")
    assert torch.equal(run.bits, _launch(lib, q, k, v, chunk=chunk).bits)


# ---- masks -----------------------------------------------------------------------------------------------------------------------------------------------

def _dominant_edges_case(B, T, H, chunk, seed):
    """Near-uniform random scores, plus a score bonus of 22 (weight x e^2.75 = 16) on the first AND the last key of every chunk (and key T - 1) against every
    query, with V = +3 on first keys and -3 on last keys: a query that sees one key past its chunk, or misses its chunk's last key, is off by ~0.1 .. 1 of
    vmax, against a bound of 2^-8 (vmax + |o|)."""
    q = _randn((B, T, H, 64), seed, 0.5); k = _randn((B, T, H, 64), seed + 1, 0.5); v = _randn((B, T, H, 64), seed + 2)
    q[..., 0] = 1.0
    j = torch.arange(T)
    c = chunk if chunk > 0 else T
    first, last = (j % c == 0), (j % c == c - 1) | (j == T - 1)
    k[:, first, :, 0] = 22.0; k[:, last, :, 0] = 22.0
    v[:, first] = 3.0 + 0.1 * v[:, first]; v[:, last] = -3.0 + 0.1 * v[:, last]
    return _bf(q), _bf(k), _bf(v)


@pytest.mark.parametrize("chunk", [13, 32, 50, 64, 100, 200])
def test_chunk_mask_edges(lib, chunk):
    """MASK_CHUNK at chunk 13 (several boundaries inside one 32-query wave, so the wave-uniform no-mask shortcut klim_min_w must come from the wave's FIRST
    query), 32 / 64 (boundaries on wave / tile edges), 50 (the CosyVoice2 estimator's), 100 and 200 >= T (no boundary); T = 193 (a partial last key tile)."""
    B, T, H = 1, 193, 2
    q, k, v = _dominant_edges_case(B, T, H, chunk, 40 + chunk)
    run = _launch(lib, q, k, v, chunk=chunk)
    _check(run, q, k, v, chunk, what="chunk=%d" % chunk)


_KLENS = [1, 2, 63, 64, 65, 128, 129, 0]          # T = 129: 1, 2, 63, 64, 65, T - 1, T, and an empty row


@pytest.mark.parametrize("chunk", [0, 13, 50])
def test_key_counts_and_padding(lib, chunk):
    """cv_attn_args.klen semantics, mixed inside one launch (klen = 1, 2, 63, 64, 65, T - 1, T and 0), alone and with the chunk mask.
    Masked content has no influence, bit for bit: K rows at or past klen[b] are filled with keys that would take all of the softmax if seen (score +200),
    their V^T columns and the pad columns [T, ldt) with 3e4 - the output bits equal those of a launch with zeros there, and both meet the fp64 bound.
    klen = 0 gives an all-zero row (the l > 0 guard).  A row with klen = n equals, for its first n queries, the same row alone at T = n, bit for bit."""
    B, T, H = len(_KLENS), 129, 2
    q, k, v = _random_case(B, T, H, 61)
    q[..., 0] = 1.0
    kf, vf = k.clone(), v.clone()
    kz, vz = k.clone(), v.clone()
    for b, n in enumerate(_KLENS):
        kf[b, n:] = 4.0; kf[b, n:, :, 0] = 200.0; vf[b, n:] = 3.0e4
        kz[b, n:] = 0.0; vz[b, n:] = 0.0
    kf, vf = _bf(kf), _bf(vf)
    filled = _launch(lib, q, kf, vf, chunk=chunk, klen=_KLENS, vt_pad=3.0e4)
    zeros = _launch(lib, q, kz, vz, chunk=chunk, klen=_KLENS)
    assert torch.equal(filled.bits, zeros.bits), "masked keys changed the output"
    _check(filled, q, kf, vf, chunk, _KLENS, what="klen, chunk=%d" % chunk)
    _check(zeros, q, kz, vz, chunk, _KLENS, what="klen zero-filled, chunk=%d" % chunk)
    assert bool((filled.o[_KLENS.index(0)] == 0).all())
    if chunk != 13:
        for b, n in enumerate(_KLENS):
            if n in (0, T):
                continue
            alone = _launch(lib, q[b:b + 1, :n].contiguous(), kz[b:b + 1, :n].contiguous(), vz[b:b + 1, :n].contiguous(), chunk=chunk)
            assert torch.equal(alone.bits, filled.bits[b * T:b * T + n]), "klen = %d differs from the same row alone at T = %d" % (n, n)


# ---- lazy rescale ----------------------------------------------------------------------------------------------------------------------------------------

def _moves(q, k, chunk=0, klen=None):
    """Per (b, query, head): how often the kernel's lazy rescale moves the running maximum AFTER the first key tile, by the kernel's rule
    (mt > m_run + 8 / (scale log2 e), scores in raw units, mt = the maximum over the visible keys of a 64-key tile), computed from the bf16 operands;
    and the smallest distance of any tile maximum from its threshold (the decisions must not hinge on fp32 rounding)."""
    B, T, H, _ = q.shape
    c2 = torch.tensor(SCALE, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    thr = THR_LOG2 / c2.double().item()
    moves = torch.zeros(B, T, H, dtype=torch.int64)
    margin = float("inf")
    for b in range(B):
        vis = _visible(T, T if klen is None else klen[b], chunk)
        s = torch.einsum("qhd,khd->hqk", q[b].double(), k[b].double()).masked_fill(~vis[None], float("-inf"))
        m_run = torch.full((H, T), float("-inf"), dtype=torch.float64)
        for t0 in range(0, T, 64):
            mt = s[:, :, t0:t0 + 64].amax(-1)
            seen = torch.isfinite(mt)
            d = mt - (m_run + thr)
            if t0 > 0 and bool(seen.any()):
                margin = min(margin, d[seen].abs().min().item())
            mv = seen & (d > 0)
            if t0 > 0:
                moves[b] += mv.T.to(torch.int64)
            m_run = torch.where(mv, mt, m_run)
    return moves, margin


def _rescale_case(T, levels, seed):
    """Scores along one direction: q = (8 sigma, noise), k = (level / 8, noise), so query (sigma = +1) sees its raw scores at the key's level (+- ~0.3 of noise) and
    query (sigma = -1) their negatives.  sigma alternates query by query: inside every 32-query wave, half the queries climb the levels, half never move."""
    H = 1
    q = _randn((1, T, H, 64), seed, 0.2); k = _randn((1, T, H, 64), seed + 1, 0.2)
    sigma = 1.0 - 2.0 * (torch.arange(T) % 2).float()
    q[0, :, 0, 0] = 8.0 * sigma
    k[0, :, 0, 0] = levels / 8.0
    return _bf(q), _bf(k)


def test_lazy_rescale_moves(lib):
    """The lazy-rescale branch with live accumulators (flow_attn32.h: a lane moves its maximum only when a tile's maximum exceeds it by more than 2^8 in
    probability; the threshold is ~44.4 in raw score units at scale 1/8).  Five key tiles: tile 0 at level 0; tile 1 a spike at 48 (move 1) over a plateau
    at 44; tile 2 the plateau; tile 3 a spike at 96 (move 2, 48 above the first) over the plateau; tile 4 the plateau.  At the end the plateau keys before
    the second move still hold ~14 % of the weight, with V regions of mean +2 (tiles 1-2) and -2 (tiles 3-4): a missing l_run *= alpha, a missing accumulator
    multiply or a stale m_s (the exponent offset not following m_run) moves the output by ~0.2 .. 100 x vmax.  Queries of sigma = -1 in the same waves never
    move (bits independent of wave mates: checked against the fp64 bound, and queries of both kinds share every wave).  The test asserts its own premise."""
    T = 320
    levels = torch.full((T,), 44.0)
    levels[:64] = 0.0
    levels[64 + 5] = 48.0
    levels[192 + 17] = 96.0
    q, k = _rescale_case(T, levels, 5)
    v = _randn((1, T, 1, 64), 9, 0.5)
    v[0, 64:192] += 2.0; v[0, 192:] -= 2.0
    v = _bf(v)
    moves, margin = _moves(q, k)
    assert margin > 0.5, margin
    for w in range(T // 32):
        mw = moves[0, 32 * w:32 * w + 32, 0]
        assert int(mw.max()) >= 2 and int(mw.min()) == 0, (w, mw.tolist())
    run = _launch(lib, q, k, v)
    _check(run, q, k, v, what="lazy rescale")


def test_lazy_rescale_just_below_threshold(lib):
    """Tile maxima that stay just below the threshold (two keys at 43.5 raw in tile 1 against ~44.4 above tile 0's maximum, a plateau at 40 in tile 2): no lane
    moves after tile 0, and the unnormalised probabilities reach ~2^7.7 ~ 200 - close to the largest the lazy scheme lets through (256), rounded to bf16 as P and
    summed unrounded in the denominator."""
    T = 192
    levels = torch.full((T,), 20.0)
    levels[:64] = 0.0
    levels[64 + 3] = 43.5; levels[64 + 40] = 43.5
    levels[128:] = 40.0
    q, k = _rescale_case(T, levels, 6)
    v = _bf(_randn((1, T, 1, 64), 10))
    moves, margin = _moves(q, k)
    assert int(moves.max()) == 0 and margin > 0.5, (int(moves.max()), margin)
    s = torch.einsum("qd,kd->qk", q[0, :, 0].double(), k[0, :, 0].double())
    m0 = s[:, :64].amax(-1)
    pmax = torch.exp2((s.amax(-1) - m0) * SCALE * 1.4426950408889634)
    assert float(pmax.max()) > 200.0, float(pmax.max())
    run = _launch(lib, q, k, v)
    _check(run, q, k, v, what="just below the threshold")


# ---- the estimator's sizes on the hardware -------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("T,chunk", [(674, 50), (1348, 0)])
def test_cfg_doubled_pass_sizes(hip_lib, T, chunk):
    """The CFG-doubled 8-utterance pass: B = 16 estimator rows, H = 8 heads, T = 674 (the U10 request, chunk mask of the streaming estimator) and 1348,
    estimator geometry, ragged klen on the first; the largest case three times, bit-identical (output determinism across the K / V^T DMA ring).
    Hardware only: the emulator pays T^2 per call."""
    lib = hip_lib
    B, H = 16, 8
    q, k, v = _random_case(B, T, H, 300 + T)
    klen = [T - 37 * b for b in range(B)] if chunk else None
    run = _launch(lib, q, k, v, chunk=chunk, klen=klen, interleave=True, ldt=_round_up(T, 64), extra_rows=1, ldo=64 * H + 4)
    _assert_untouched(run, B, T, H)
    _check(run, q, k, v, chunk, klen, what="T=%d" % T)
    if T == 1348:
        for _ in range(2):
            assert torch.equal(_launch(lib, q, k, v, chunk=chunk, klen=klen, interleave=True, ldt=_round_up(T, 64), extra_rows=1, ldo=64 * H + 4).bits, run.bits)


# ---- argument checks -------------------------------------------------------------------------------------------------------------------------------------

def test_arguments_are_checked(lib):
    """Each refused argument returns an error (CosyVoiceAmdError with cv_last_error), nothing is launched."""
    dev = lib.device
    B, T, H = 1, 40, 2
    HD, ldt = 64 * H, 64
    buf = lib.hook(torch.zeros(4 * B * T * HD + 64, dtype=torch.bfloat16).to(dev))
    vt = lib.hook(torch.zeros(B * HD * ldt + 64, dtype=torch.bfloat16).to(dev))
    o = lib.hook(torch.zeros(B * T * HD + 64, dtype=torch.bfloat16).to(dev))
    good = dict(q=buf.data_ptr(), k=buf.data_ptr() + 2 * B * T * HD * 2, ld=HD, vt=vt.data_ptr(), vt_batch=HD * ldt, ldt=ldt, o=o.data_ptr(), ldo=HD,
                B=B, H=H, T=T, scale=SCALE, chunk=0, waves=0)

    def call(**kw):
        a = dict(good, **kw)
        lib.cv_flow_attention_bf16(C.c_void_p(a["q"]), C.c_void_p(a["k"]), C.c_int32(a["ld"]), C.c_void_p(a["vt"]), C.c_int64(a["vt_batch"]), C.c_int32(a["ldt"]),
                                   C.c_void_p(a["o"]), C.c_int32(a["ldo"]), C.c_int32(a["B"]), C.c_int32(a["H"]), C.c_int32(a["T"]), C.c_float(a["scale"]),
                                   C.c_int32(a["chunk"]), None, C.c_int32(a["waves"]), stream_ptr(lib))
        _sync(lib)

    call()                                                       # the reference point: accepted
    bad = [dict(q=None), dict(k=None), dict(vt=None), dict(o=None), dict(B=0), dict(H=0), dict(T=0), dict(T=-3),
           dict(ld=HD + 4), dict(ld=HD - 8), dict(ldo=HD + 2), dict(ldo=HD - 4), dict(ldt=96), dict(ldt=0), dict(T=65), dict(vt_batch=HD * ldt - 1),
           dict(q=good["q"] + 8), dict(k=good["k"] + 2), dict(vt=good["vt"] + 8), dict(o=good["o"] + 4),
           dict(scale=0.0), dict(scale=-0.125), dict(scale=float("inf")), dict(scale=float("nan")), dict(chunk=-1), dict(waves=1), dict(waves=3), dict(waves=8)]
    for kw in bad:
        with pytest.raises(CosyVoiceAmdError, match="cv_flow_attention_bf16"):
            call(**kw)
