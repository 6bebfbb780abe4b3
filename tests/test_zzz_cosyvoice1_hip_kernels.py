"""The kernels of the CosyVoice-300M decode step (csrc/lm1.hip: lm1_attn_kernel, the forms of lm1_gemv_kernel / lm1_gemv16_kernel for the single sequence and for the slots of the batch) against float64
references, through the test entry points cv_lm1_attention, cv_lm1_gemv and cv_lm1_gemv_batch - the launch helpers of the step itself (launch_attn, gemv() for the single sequence and for the slots).

Every operand is allocated at its exact size through lib.hook (under the emulator it ends flush against an inaccessible page); outputs carry a sentinel and spare tail
elements, and exactly the problem's elements must have been written.  U = 2^-24 below.

ATTENTION.  Reference: float64 from the fp32 operands, score_j = ((q + u) . k_j + (q + v) . p_(n - 1 - j)) scale, softmax, P . V; the table contract is restated here
(row m of a [2 n_tab - 1][d] table is relative position n_tab - 1 - m, so key j of n reads row n_tab - n + j).  Two comparisons per case: (a) the kernel's 8 partials per
head merged in float64 inside the test, (b) the partials fed through the production MERGE prologue (cv_lm1_gemv with an identity matrix: products and sums with 0 are
exact, y is the merged vector); (b) must also agree with (a) to 32 U vmax (weights w / L: expf, an 8-term sum, a division; then an 8-term sum of products).
Bound (derived).  A score is two 64-term dot products, each 4 products chained in a lane and a 4-step group reduction (8 dependent roundings), added and scaled:
|ds_j| <= 10 U A_j, A_j = (sum |(q+u) k_j| + sum |(q+v) p_j|) scale.  A weight e^(s_j - M) goes through up to three exponentials (the key's own, the alpha chain or the
16-group merge, the merge of the 8 ranges); each adds the rounding of its argument (<= 40 U for any weight above e^-40 of the largest; smaller ones weigh nothing) and
the expf error E = 4 ulp.  The sums: a lane group adds ceil(per / 16) keys and rescales once per sweep, the group merge adds 16 terms, the range merge 8, each with a
product: kpg + 2 sweeps + 28.  A relative weight error r moves the quotient by at most r (vmax + |ref|), so per element
    |o - ref| <= C U G (vmax + |ref|),   G = 10 max_j A_j + 3 (40 + E) + kpg + 2 sweeps + 28,   vmax = max |v| over the visible keys of the head.
C covers what cannot be derived (the device expf): the same reference evaluated in float32 on the CPU with the keys permuted (test_fp32_reference_sits_inside_the_bound)
reaches at most 0.039 of U G (vmax + |ref|) over the cases of this file (measured); 4 x that is 0.16, below 1, so C = max(1, 0.16) = 1: G alone, a worst-case count, is the bound.
The constructions below miss a wrong kernel by 1e-2 .. 1e2 of vmax against bounds of 1e-5 .. 1e-4 (vmax + |ref|).

GEMV.  Reference: float64 from the operands (bf16 matrices widened; LayerNorm and the merge in float64), then bias, act, res.
    |y - ref| <= (c + 2) U (sum_k |w_k x_k| + |bias| + |res|) + prologue term + activation term
c = the longest chain of dependent additions of the form gemv() selects (_chain): the lane's own products, the 4-step group reduction, the combine of the waves.  Never K:
at K = 4096 a K-term bound is as large as one missing product.  Operands have magnitudes in [0.5, 1.5] and random signs, and each test asserts that the smallest
single product exceeds the bound tenfold (a dropped, duplicated or misplaced element cannot hide).  LayerNorm prologue (fp32 mean over a 22-deep chain, centred squares,
rsqrtf at 4 ulp): |d mean| <= 23 U mean|x|; rstd relative error r = 20 U + (d mean / sigma)^2 / 2; per element |d ln_k| <= |g_k| ((d mean + U |x_k - mean|) / sigma +
|xhat_k| (r + 3 U)) + U |ln_k|, carried through |W|.  Merge prologue: 32 U sum_s |acc_s| w_s / L per element (as above), carried through |W|.  SiLU (fast_exp = exp2 of a
scaled argument, a hardware reciprocal): relative 2 (|t| + 8) U on top of 1.1 x the bound of its argument t; ReLU is exact.

Which kernel form a shape selects is restated from gemv() in _form() (the test ids carry it; there is no cheap way to observe the choice from outside).

Mutants of csrc/lm1.hip that each fail this file under the emulator are listed in the commit that added it.
Emulator share of this file: about 45 s on one worker."""
import ctypes as C

import pytest
import torch

from cosyvoice_amd._lib import ACT, CosyVoiceAmdError, Lm1Config, Lm1LayerBf16, Lm1LayerWeights, stream_ptr

U = 2.0 ** -24
SCALE = 0.125
SENT = -1.2345e30                  # what an unwritten output element holds
TAIL = 16                          # spare output elements behind the problem's (a workgroup of the whole-row forms spans 16 rows)
E_EXP = 4.0                        # expf / rsqrtf error allowance in ulp
C_ATTN = 1.0                       # see the module docstring: max(1, 4 x the float32 reference's ratio)
NONE, LN, MERGE = 0, 1, 2
i32, i64, u32, f32 = C.c_int32, C.c_int64, C.c_uint32, C.c_float


def _sync(lib):
    if not lib.emulated:
        torch.cuda.synchronize()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _dev(lib, t):
    return None if t is None else lib.hook(t.contiguous().to(lib.device))


def _p(t):
    return C.c_void_p(None if t is None else t.data_ptr())


def _sent(n):
    return torch.full((n,), SENT, dtype=torch.float32)


_S32 = float(torch.tensor(SENT, dtype=torch.float32))

# ---- a handle for the GEMV hooks (its model weights do not matter) ---------------------------------------------------------------------------------------------

_handles = {}


def _make_handle(lib, keep):
    """A zero-weight handle (d = 64, one layer); `keep` holds its tensors."""
    d, ffn, n_out = 64, 128, 10

    def buf(*shape):
        keep.append(torch.zeros(*shape).to(lib.device))
        return keep[-1].data_ptr()
    lw = (Lm1LayerWeights * 1)()
    for name, shape in (("ln1_g", (d,)), ("ln1_b", (d,)), ("w_qkv", (4 * d, d)), ("b_qkv", (4 * d,)), ("w_out", (d, d)), ("b_out", (d,)), ("ln2_g", (d,)), ("ln2_b", (d,)),
                        ("w1", (ffn, d)), ("b1", (ffn,)), ("w2", (d, ffn)), ("b2", (d,))):
        setattr(lw[0], name, buf(*shape))
    c = Lm1Config()
    c.n_layers, c.d, c.heads, c.ffn, c.d_in, c.n_out, c.act, c.xscale = 1, d, 1, ffn, d, n_out, ACT["relu"], 8.0
    for name, shape in (("embed_w", (d, d)), ("embed_b", (d,)), ("embed_g", (d,)), ("embed_beta", (d,)), ("after_g", (d,)), ("after_b", (d,)), ("dec_w", (n_out, d)), ("dec_b", (n_out,))):
        setattr(c, name, buf(*shape))
    h = C.c_void_p(lib.raw("cv_lm1_create", C.c_void_p)(C.byref(c), lw))
    assert h
    return h


def _handle(lib):
    """One handle per library for the GEMV hooks, in bf16 mode (gemv() takes the bf16 kernels when W16 is given and the handle's w16 flag is set, as in production)."""
    if id(lib) not in _handles:
        keep, d, ffn = [], 64, 128
        h = _make_handle(lib, keep)
        l16 = (Lm1LayerBf16 * 1)()
        for name, shape in (("w_qkv", (4 * d, d)), ("w_out", (d, d)), ("w1", (ffn, d)), ("w2", (d, ffn))):
            keep.append(torch.zeros(*shape, dtype=torch.bfloat16).to(lib.device))
            setattr(l16[0], name, keep[-1].data_ptr())
        lib.cv_lm1_use_bf16(h, l16, None, None)
        _handles[id(lib)] = (h, keep)
    return _handles[id(lib)][0]


# =================================================================================================================================================================
# attention
# =================================================================================================================================================================

class Case:
    """One sequence: cache rows [n][4 d] = (q + u | q + v | k | v) (the query is the last row), table [2 n_tab - 1][d]."""

    def __init__(self, rows, tab, n_tab, H):
        self.rows, self.tab, self.n_tab, self.H = rows.float().contiguous(), tab.float().contiguous(), n_tab, H
        self.n, self.d = rows.shape[0], 64 * H
        assert rows.shape[1] == 4 * self.d and tab.shape == (2 * n_tab - 1, self.d) and n_tab >= self.n


def _attn_launch(lib, cases, nb):
    """cv_lm1_attention on `cases` (None = an inactive slot: null pointers) -> the partials [max(nb, 1)][H][8][66] and the tail behind them."""
    n_slots = max(nb, 1)
    live = [c for c in cases if c is not None]
    H, d = live[0].H, live[0].d
    keep = [(None, None) if c is None else (_dev(lib, c.rows), _dev(lib, c.tab)) for c in cases]
    rows = (C.c_void_p * n_slots)(*[None if r is None else r.data_ptr() for r, _ in keep])
    tabs = (C.c_void_p * n_slots)(*[None if t is None else t.data_ptr() for _, t in keep])
    n_tab = (i32 * n_slots)(*[0 if c is None else c.n_tab for c in cases])
    pos = (i32 * n_slots)(*[-1 if c is None else c.n - 1 for c in cases])
    part = _dev(lib, _sent(n_slots * H * 8 * 66 + TAIL))
    lib.cv_lm1_attention(i32(nb), rows, tabs, n_tab, pos, i32(d), i32(H), f32(SCALE), _p(part), stream_ptr(lib))
    _sync(lib)
    out = part.cpu().clone()
    assert bool((out[n_slots * H * 8 * 66:] == _S32).all()), "a write behind the partials"
    return out[:n_slots * H * 8 * 66].reshape(n_slots, H, 8, 66)


def _attn_ref(c, dtype=torch.float64, perm=None):
    """-> scores [n][H], out [H][64], vmax [H], A [H] (the largest sum of absolute score terms), in `dtype`; perm: the keys in another order (the float32 yardstick)."""
    n, d, H = c.n, c.d, c.H
    r, t = c.rows.to(dtype), c.tab.to(dtype)
    qu, qv = r[n - 1, :d], r[n - 1, d:2 * d]
    k, v = r[:, 2 * d:3 * d], r[:, 3 * d:]
    p = t[c.n_tab - n + torch.arange(n)]                       # key j sits at relative position n - 1 - j = table row n_tab - 1 - (n - 1 - j)
    if perm is not None:
        k, v, p = k[perm], v[perm], p[perm]
    tk, tp = (qu * k).reshape(n, H, 64), (qv * p).reshape(n, H, 64)
    s = (tk.sum(-1) + tp.sum(-1)) * SCALE
    A = ((tk.abs().sum(-1) + tp.abs().sum(-1)) * SCALE).amax(0)
    w = torch.softmax(s, 0)
    out = torch.einsum("jh,jhd->hd", w, v.reshape(n, H, 64))
    vmax = v.abs().reshape(n, H, 64).amax((0, 2))
    return s, out, vmax, A


def _attn_bound(c, out, vmax, A):
    per = (c.n + 7) // 8
    G = 10.0 * A.double() + 3 * (40 + E_EXP) + (per + 15) // 16 + 2 * ((per + 63) // 64) + 28
    return C_ATTN * U * G[:, None] * (vmax.double()[:, None] + out.double().abs())


def _merge64(part):
    """[H][8][66] partials -> [H][64]: sum acc_s e^(m_s - M) / sum l_s e^(m_s - M) in float64."""
    p = part.double()
    m, l, acc = p[..., 0], p[..., 1], p[..., 2:]
    w = torch.exp(m - m.amax(-1, keepdim=True)).nan_to_num(0.0)
    return (acc * w[..., None]).sum(1) / (l * w).sum(1)[:, None]


def _merge_through_gemv(lib, part, H):
    """The partials through the production MERGE prologue: cv_lm1_gemv(pro = MERGE, W = identity, no bias, no res) -> the merged vector [H][64]."""
    d = 64 * H
    x = _dev(lib, part.reshape(-1).float())
    W = _dev(lib, torch.eye(d))
    y = _dev(lib, _sent(d + TAIL))
    lib.cv_lm1_gemv(_handle(lib), i32(MERGE), _p(x), None, None, f32(0.0), _p(W), None, None, None, _p(y), i32(d), i32(d), i32(ACT["none"]), stream_ptr(lib))
    _sync(lib)
    y = y.cpu().clone()
    assert bool((y[d:] == _S32).all()) and not bool((y[:d] == _S32).any())
    return y[:d].reshape(H, 64)


def _check_part(lib, c, part, what):
    """part [H][8][66] of case c against the float64 reference, both ways; the empty ranges report (-inf, 0)."""
    assert not bool((part == _S32).any()), "%s: an element of the partials was not written" % what
    per = (c.n + 7) // 8
    for s in range(8):
        if s * per >= c.n:
            assert bool((part[:, s, 0] == float("-inf")).all()) and bool((part[:, s, 1:] == 0).all()), "%s: empty range %d does not report (-inf, 0, 0)" % (what, s)
        else:
            assert bool(torch.isfinite(part[:, s]).all()), (what, s)
    _, ref, vmax, A = _attn_ref(c)
    bound = _attn_bound(c, ref, vmax, A)
    a = _merge64(part)
    b = _merge_through_gemv(lib, part, c.H).double()
    for name, got in (("float64 merge", a), ("MERGE prologue", b)):
        err = (got - ref).abs()
        worst = (err / bound).flatten().argmax().item()
        print("%s [%s]: max err / bound = %.3g (err %.3g, bound %.3g)" % (what, name, (err / bound).max().item(), err.flatten()[worst].item(), bound.flatten()[worst].item()))
        assert bool((err <= bound).all()), "%s [%s]: |o - ref| above the bound at %d: err %.4g, bound %.4g, ref %.4g" % (
            what, name, worst, err.flatten()[worst].item(), bound.flatten()[worst].item(), ref.flatten()[worst].item())
    assert bool(((a - b).abs() <= 32 * U * vmax.double()[:, None]).all()), "%s: the MERGE prologue and the float64 merge of the same partials differ by %.3g" % (what, (a - b).abs().max().item())
    return ref


def _run_case(lib, c, what):
    part = _attn_launch(lib, [c], 0)[0]
    return part, _check_part(lib, c, part, what)


def _random_case(n, H, seed, n_tab=None):
    n_tab = n_tab or n
    g = _gen(seed)
    return Case(torch.randn(n, 256 * H, generator=g), torch.randn(2 * n_tab - 1, 64 * H, generator=g), n_tab, H)


_NS = [1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 511, 512, 513, 520, 576, 577, 1024, 1025, 1032, 1100]


def _key_count_case(n):
    return _random_case(n, 1 + _NS.index(n) % 2, 1000 + n, n_tab=n + (5 if n % 2 else 0))


@pytest.mark.parametrize("n", _NS)
def test_attention_key_counts(lib, n):
    """n keys over the 8 ranges: empty and partial last ranges (n < 8, 9, 17 ...), the first key of a second sweep (513: one live lane group, fifteen idle ones
    that must keep their state), a full second sweep (1024), the third sweep (1025 .. 1100).  Random operands, H = 1 and 2 alternating, n_tab = n and n + 5."""
    _run_case(lib, _key_count_case(n), "n=%d" % n)


# ---- rescale ---------------------------------------------------------------------------------------------------------------------------------------------------

def _where(n):
    """The kernel's key -> (range, lane group, sweep) rule: range s holds keys [s per, s per + per), key i of a range goes to group i % 16 in sweep i // 64."""
    per = (n + 7) // 8
    j = torch.arange(n)
    i = j % per
    return j // per, i % 16, i // 64


def _moves(c):
    """Per (range, group): how often the running maximum moves AFTER the group's first sweep with a key, from the float64 scores; and the smallest distance of a
    sweep's maximum from the running maximum it is compared with (no decision may hinge on fp32 rounding)."""
    s = _attn_ref(c)[0][:, 0]
    rng, grp, swp = _where(c.n)
    moves, margin = torch.zeros(8, 16, dtype=torch.int64), float("inf")
    for r in range(8):
        for g in range(16):
            m_run = None
            for t in range(int(swp.max()) + 1):
                sel = (rng == r) & (grp == g) & (swp == t)
                if not bool(sel.any()):
                    continue
                mt = float(s[sel].max())
                if m_run is not None:
                    margin = min(margin, abs(mt - m_run))
                    if mt > m_run:
                        moves[r, g] += 1
                m_run = mt if m_run is None else max(m_run, mt)
    return moves, margin


def _level_case(n, levels, vmean, seed):
    """H = 1; scores along one direction: (q + u)[0] = 8, k_j[0] = level_j (score = level_j, + ~0.1 of noise from the other dimensions and the table); V = vmean_j + noise."""
    g = _gen(seed)
    rows = torch.randn(n, 256, generator=g) * 0.1
    rows[n - 1, 0] = 8.0
    rows[:, 128] = levels
    rows[:, 192:] = vmean[:, None] + 0.3 * torch.randn(n, 64, generator=g)
    return Case(rows, torch.randn(2 * n - 1, 64, generator=g) * 0.1, n, 1)


def _rescale_case():
    n = 1104
    _, grp, swp = _where(n)
    i = torch.arange(n) % (n // 8)
    levels = torch.where(grp < 12, 5.0 * swp, 10.0 - 5.0 * swp).float()
    levels[i == 64 + 16 + 3] = 9.0
    levels[i == 128 + 5] = 14.0
    return _level_case(n, levels, torch.tensor([2.0, -2.0, 1.0])[swp], 11)


def test_attention_rescale_with_live_accumulators(lib):
    """n = 1104: 138 keys per range = sweeps of 64, 64 and 10 keys.  Lane groups 0 .. 11 climb (plateaus at 0, 5, 10 sweep by sweep; a spike at 9 in sweep 1 and a
    higher one at 14 in sweep 2): groups 0 .. 9 move their maximum twice, 10 and 11 once.  Groups 12 .. 15 descend (10, then 5): they never move, in the same
    workgroup.  V has mean +2 in sweep 0, -2 in sweep 1, +1 in sweep 2, and the keys seen before a move keep a visible share of the weight at the end:
    a missing l_run *= alpha, a missing accumulator rescale or a stale m_run moves the result by 0.1 .. 10 vmax."""
    c = _rescale_case()
    _, grp, swp = _where(c.n)
    moves, margin = _moves(c)
    assert margin > 0.5, margin
    for r in range(8):
        assert int(moves[r, :10].min()) == 2 and moves[r, 10:12].tolist() == [1, 1] and int(moves[r, 12:].max()) == 0, (r, moves[r].tolist())
    # the premise on visibility: what the climbing groups saw before their last move is a visible share of the whole
    w = torch.softmax(_attn_ref(c)[0][:, 0], 0)
    early = float(w[(grp < 12) & (swp < 2)].sum())
    assert early > 0.003, early
    _run_case(lib, c, "rescale")


def test_attention_maximum_in_the_first_sweep(lib):
    """The mirror: every group's maximum sits in sweep 0 (level 100) and the later keys are 100 below it - their e underflows to (nearly) 0, alpha = expf(0) = 1, the
    running state must pass through the later sweeps unchanged."""
    n = 1100
    _, _, swp = _where(n)
    c = _level_case(n, torch.where(swp == 0, 100.0, 0.0), torch.tensor([2.0, -2.0, 1.0])[swp], 12)
    moves, margin = _moves(c)
    assert int(moves.max()) == 0 and margin > 50, (int(moves.max()), margin)
    _run_case(lib, c, "maximum in sweep 0")


def test_attention_group_maxima_far_apart(lib):
    """The 16 group maxima of a range 7 apart (0 .. 105): the lower groups' weights underflow in the LDS merge."""
    n = 300
    _, grp, _ = _where(n)
    c = _level_case(n, 7.0 * grp.float(), torch.where(grp % 2 == 0, 2.0, -2.0), 13)
    s = _attn_ref(c)[0][:, 0]
    rng = _where(n)[0]
    gmax = torch.stack([s[(rng == 0) & (grp == g)].max() for g in range(16)])
    assert float(gmax.max() - gmax.min()) > 90
    _run_case(lib, c, "group maxima 105 apart")


def test_attention_one_range_dominates(lib):
    """Range 3 sits 100 above the other seven: their weights underflow in the MERGE prologue (and in the float64 merge), the result is range 3's alone."""
    n = 300
    rng = _where(n)[0]
    c = _level_case(n, torch.where(rng == 3, 100.0, 0.0), torch.where(rng == 3, -2.0, 2.0), 14)
    part = _run_case(lib, c, "one range dominates")[0]
    assert float(part[0, 3, 0] - part[0, [0, 1, 2, 4, 5, 6, 7], 0].max()) > 90


# ---- relative positions ----------------------------------------------------------------------------------------------------------------------------------------

def _position_case(n, n_tab, seed):
    """k = 0 in the cache: only (q + v) . p carries signal.  The table rows of relative position 0 (key n - 1) and n - 1 (key 0) score 12, with V = +3 and -2 there;
    the rows just outside the n positions in use (relative position -1 and n) score 30: a kernel that touches them, or is one row off, changes the result by ~vmax."""
    g = _gen(seed)
    rows = torch.randn(n, 256, generator=g)
    rows[:, 128:192] = 0.0
    rows[n - 1, 64:128] = 0.1 * torch.randn(64, generator=g)
    rows[n - 1, 64] = 8.0
    rows[n - 1, 192:] = 3.0 + 0.1 * rows[n - 1, 192:]
    rows[0, 192:] = -2.0 + 0.1 * rows[0, 192:]
    tab = torch.randn(2 * n_tab - 1, 64, generator=g) * 0.5
    tab[:, 0] = 0.0

    def row_of(rel):
        return n_tab - 1 - rel
    tab[row_of(0), 0] = 12.0
    tab[row_of(n - 1), 0] = 12.0
    tab[row_of(-1), 0] = 30.0 if n_tab > 1 else 12.0
    if n < n_tab:
        tab[row_of(n), 0] = 30.0
    return Case(rows, tab, n_tab, 1)


@pytest.mark.parametrize("n,n_tab", [(577, 577), (577, 614), (577, 1024), (9, 9), (9, 46), (9, 16)])
def test_attention_position_term_alone(lib, n, n_tab):
    """tab + (n_tab - n) d: n_tab = n (the cap edge: the first table row is in use), n + 37 and a power of two above n.  The expected result is the mean of the two
    dominant keys' V (+3 and -2) to ~1e-3; a table shifted by one row either way gives neither (asserted on the reference itself: the premise)."""
    c = _position_case(n, n_tab, 20 + n_tab)
    ref = _run_case(lib, c, "position n=%d n_tab=%d" % (n, n_tab))[1]
    assert bool(((ref - 0.5).abs() < 0.5).all())                 # neither dominant key alone (+3 or -2)
    _, out, vmax, A = _attn_ref(c)
    for shift in (-1, 1):
        moved = Case(c.rows, torch.roll(c.tab, shift, 0), n_tab, 1)
        miss = (_attn_ref(moved)[1] - out).abs().median()         # (the median over the 64 elements: V rows are random, single elements may coincide)
        assert float(miss) > 1000 * float(_attn_bound(c, out, vmax, A).max()), (shift, float(miss))


@pytest.mark.parametrize("n", [9, 577])
def test_attention_key_term_alone(lib, n):
    """The mirror: table = 0, dominant keys at j = 0 and j = n - 1 through k."""
    g = _gen(40 + n)
    rows = torch.randn(n, 256, generator=g)
    rows[:, 128:192] *= 0.5
    rows[:, 128] = 0.0
    rows[n - 1, :64] = 0.1 * torch.randn(64, generator=g)
    rows[n - 1, 0] = 8.0
    rows[0, 128] = 12.0
    rows[n - 1, 128] = 12.0
    rows[n - 1, 192:] = 3.0 + 0.1 * rows[n - 1, 192:]
    rows[0, 192:] = -2.0 + 0.1 * rows[0, 192:]
    ref = _run_case(lib, Case(rows, torch.zeros(2 * n - 1, 64), n, 1), "key term n=%d" % n)[1]
    assert bool(((ref - 0.5).abs() < 0.5).all())                 # neither dominant key alone (+3 or -2)


# ---- the batched grid ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nb,where", [(3, {0: 9, 2: 577}), (8, {7: 65})], ids=["nb3-middle-empty", "nb8-last-only"])
def test_attention_batched_grid(lib, nb, where):
    """blockIdx.z = slot: inactive slots (null pointers) leave their block of `part` untouched, every active slot has the bits of the single-sequence launch."""
    cases = [_random_case(where[i], 2, 70 + i, n_tab=where[i] + 3 * i) if i in where else None for i in range(nb)]
    part = _attn_launch(lib, cases, nb)
    for i, c in enumerate(cases):
        if c is None:
            assert bool((part[i] == _S32).all()), "slot %d is inactive and was written" % i
        else:
            assert torch.equal(part[i], _attn_launch(lib, [c], 0)[0]), "slot %d differs from the single launch" % i
            _check_part(lib, c, part[i], "slot %d of %d" % (i, nb))


@pytest.mark.gpu
def test_attention_full_width_long_context(hip_lib):
    """d = 1024, 16 heads, 2000 keys (four sweeps per range), random operands; three runs, bit-identical.  Hardware only."""
    c = _random_case(2000, 16, 99, n_tab=2048)
    part = _run_case(hip_lib, c, "d=1024 n=2000")[0]
    for _ in range(2):
        assert torch.equal(_attn_launch(hip_lib, [c], 0)[0], part)


def _attention_cases():
    """Every attention case of this file that the float32 yardstick is taken over (the random ones and the constructions)."""
    out = [_key_count_case(n) for n in _NS] + [_rescale_case()]
    n = 1100
    _, grp, swp = _where(n)
    out.append(_level_case(n, torch.where(swp == 0, 100.0, 0.0), torch.tensor([2.0, -2.0, 1.0])[swp], 12))
    _, grp, _ = _where(300)
    out.append(_level_case(300, 7.0 * grp.float(), torch.where(grp % 2 == 0, 2.0, -2.0), 13))
    out += [_position_case(577, 614, 20 + 614), _random_case(2000, 16, 99, n_tab=2048)]
    return out


def test_fp32_reference_sits_inside_the_bound():
    """The constant of the attention bound is measured against the REFERENCE, never the kernel: the same reference in float32 on the CPU with the keys in a permuted
    order, against the float64 result.  4 x the largest ratio must not exceed C_ATTN (the kernel's is a third summation order; the device expf may differ by a couple of ulp)."""
    worst = 0.0
    for c in _attention_cases():
        _, ref, vmax, A = _attn_ref(c)
        got = _attn_ref(c, torch.float32, torch.randperm(c.n, generator=_gen(c.n)))[1].double()
        worst = max(worst, float(((got - ref).abs() / _attn_bound(c, ref, vmax, A)).max()) * C_ATTN)
    print("float32 reference: largest err / (U G (vmax + |ref|)) = %.4g" % worst)
    assert 4 * worst <= C_ATTN, worst


# =================================================================================================================================================================
# GEMV
# =================================================================================================================================================================

def _kp(K):
    return (K + 31) // 32 * 32


def _form(N, K, bf16, pro, wide=1, wide16=1):
    """gemv()'s dispatch rule (csrc/lm1.hip pick_form), restated: kp = K rounded up to 32, steps = 64-float steps of a row.  The strings are labels of the forms only:
    gemv<4,4> / <8,8> / <8,4> are LM1_U4 / LM1_U8_NW8 / LM1_U8 of lm1_gemv_kernel, gemv16<..> the four forms of lm1_gemv16_kernel."""
    kp = _kp(K)
    steps = (kp + 63) // 64
    if bf16 and wide16 and kp % 128 == 0:
        st = kp // 128
        if st <= 8 and N >= 2048:
            return "gemv16<bf16,8,1,4,whole>"
        if st <= 8:
            return "gemv16<bf16,2,1,4,ksplit>"
        if st <= 32 and pro == NONE:
            return "gemv16<bf16,4,1,8,ksplit>"
    if not bf16 and wide and kp % 64 == 0 and kp <= 1024 and N >= 2048:
        return "gemv16<f32,16,1,4,whole>"
    dt = "bf16" if bf16 else "f32"
    if steps <= 16:
        return "gemv<4,4,%s>" % dt
    if pro == NONE and N <= 2048:
        return "gemv<8,8,%s>" % dt
    return "gemv<8,4,%s>" % dt


def _chain(form, K):
    """The longest chain of dependent additions of a form: the lane's own products, the 4-step reduction of the 16-lane group, the combine of the waves."""
    kp = _kp(K)
    steps = (kp + 63) // 64
    if form.startswith("gemv16<f32"):
        return 4 * (kp // 64) + 4
    if form.endswith("whole>"):
        return 8 * (kp // 128) + 4
    if form.startswith("gemv16<bf16,2"):
        return 8 * -(-(kp // 128) // 4) + 4 + 4
    if form.startswith("gemv16<bf16,4"):
        return 8 * -(-(kp // 128) // 8) + 4 + 8
    nw = 8 if form.startswith("gemv<8,8") else 4
    return 4 * -(-steps // nw) + 4 + nw - 1


def _mag(shape, g):
    """Magnitudes in [0.5, 1.5], random signs."""
    return (0.5 + torch.rand(shape, generator=g)) * (1.0 - 2.0 * torch.randint(0, 2, shape, generator=g).float())


class Gemv:
    """One product's operands (host fp32 / bf16-exact fp32) and its float64 reference."""

    def __init__(self, N, K, seed, bf16=False, pro=NONE, act="none", bias=True, res=True, eps=1e-5, stiff=False, pad=0.0):
        g = _gen(seed)
        self.N, self.K, self.kp, self.bf16, self.pro, self.act, self.eps = N, K, _kp(K), bf16, pro, act, eps
        W = _mag((N, K), g)
        if bf16:
            W = W.to(torch.bfloat16).float()
        self.W = torch.full((N, self.kp), pad)
        self.W[:, :K] = W
        self.bias = _mag((N,), g) if bias else None
        self.res = _mag((N,), g) if res else None
        self.g = self.b = None
        if pro == LN:
            self.x = (100.0 + 0.1 * _mag((K,), g)) if stiff else _mag((K,), g)
            self.g = (1.0 + 0.5 * torch.rand(K, generator=g)) * (1.0 - 2.0 * torch.randint(0, 2, (K,), generator=g).float())
            self.b = 0.1 * _mag((K,), g)
        elif pro == MERGE:
            heads = K // 64
            m = 10.0 * torch.randn(heads, 8, generator=g)
            m[:, 1] = float("-inf")                              # an empty range: (-inf, 0, 0)
            m[:, 5] = m[:, 0] - 95.0                             # maxima more than 90 apart
            m[heads - 1, 6:] = float("-inf")
            l = 1.0 + 4.0 * torch.rand(heads, 8, generator=g)
            sign = 1.0 - 2.0 * torch.randint(0, 2, (heads, 1, 64), generator=g).float()
            acc = sign * (0.5 + torch.rand(heads, 8, 64, generator=g)) * l[..., None]
            empty = torch.isinf(m)
            l[empty] = 0.0
            acc[empty] = 0.0
            self.x = torch.cat([m[..., None], l[..., None], acc], -1).reshape(-1)
        else:
            self.x = _mag((K,), g)

    def reference(self, form):
        """-> (ref [N], bound [N], smallest |w_k x_k|) in float64."""
        W, K = self.W[:, :self.K].double(), self.K
        dx = torch.zeros(K, dtype=torch.float64)
        if self.pro == LN:
            x = self.x.double()
            mean = x.mean()
            var = ((x - mean) ** 2).mean()
            sigma = torch.sqrt(var + self.eps)
            xhat = (x - mean) / sigma
            xv = xhat * self.g.double() + self.b.double()
            dmean = 23 * U * x.abs().mean()
            r = 20 * U + 0.5 * (dmean / sigma) ** 2
            dx = self.g.double().abs() * ((dmean + U * (x - mean).abs()) / sigma + xhat.abs() * (r + 3 * U)) + U * xv.abs()
        elif self.pro == MERGE:
            p = self.x.double().reshape(K // 64, 8, 66)
            m, l, acc = p[..., 0], p[..., 1], p[..., 2:]
            w = torch.exp(m - m.amax(-1, keepdim=True)).nan_to_num(0.0)
            L = (l * w).sum(1)
            xv = ((acc * w[..., None]).sum(1) / L[:, None]).reshape(-1)
            dx = 32 * U * ((acc.abs() * w[..., None]).sum(1) / L[:, None]).reshape(-1)
        else:
            xv = self.x.double()
        t = W @ xv
        S = W.abs() @ xv.abs()
        bound = (_chain(form, K) + 2) * U * S + W.abs() @ dx
        if self.bias is not None:
            t = t + self.bias.double()
            bound = bound + (_chain(form, K) + 2) * U * self.bias.double().abs()
        if self.act == "relu":
            t = t.clamp(min=0.0)
        elif self.act == "silu":
            t0 = t
            t = t0 * torch.sigmoid(t0)
            bound = 1.1 * bound + 2 * (t0.abs() + 8) * U * t.abs()
        if self.res is not None:
            t = t + self.res.double()
            bound = bound + (_chain(form, K) + 2) * U * self.res.double().abs() + U * t.abs()
        return t, bound, float((W.abs() * xv.abs()[None]).min())

    def device(self, lib):
        W = self.W.to(torch.bfloat16) if self.bf16 else self.W
        return dict(x=_dev(lib, self.x), W=_dev(lib, W), bias=_dev(lib, self.bias), res=_dev(lib, self.res), g=_dev(lib, self.g), b=_dev(lib, self.b))

    def launch(self, lib, ops=None):
        """cv_lm1_gemv -> y [N] (float32 bits); the tail behind y keeps the sentinel, every element of y is written."""
        o = ops or self.device(lib)
        y = _dev(lib, _sent(self.N + TAIL))
        lib.cv_lm1_gemv(_handle(lib), i32(self.pro), _p(o["x"]), _p(o["g"]), _p(o["b"]), f32(self.eps), _p(None if self.bf16 else o["W"]), _p(o["W"] if self.bf16 else None),
                        _p(o["bias"]), _p(o["res"]), _p(y), i32(self.N), i32(self.K), i32(ACT[self.act]), stream_ptr(lib))
        _sync(lib)
        y = y.cpu().clone()
        assert bool((y[self.N:] == _S32).all()), "a write behind y[N]"
        assert not bool((y[:self.N] == _S32).any()), "an element of y was not written"
        return y[:self.N]

    def check(self, y, form, what, significant=True):
        ref, bound, smallest = self.reference(form)
        err = (y.double() - ref).abs()
        worst = (err / bound).argmax().item()
        print("%s: max err / bound = %.3g (err %.3g, bound %.3g), smallest product %.3g" % (what, float((err / bound).max()), float(err[worst]), float(bound[worst]), smallest))
        if significant:
            assert smallest > 10 * float(bound.max()), "%s: the smallest product %.3g does not stand out of the bound %.3g" % (what, smallest, float(bound.max()))
        assert bool((err <= bound).all()), "%s: |y - ref| above the bound at row %d: err %.4g, bound %.4g, ref %.4g" % (what, worst, float(err[worst]), float(bound[worst]), float(ref[worst]))


class _options:
    """Handle options for the length of a with-block (the handle is shared by the file)."""

    def __init__(self, lib, **kw):
        self.lib, self.kw = lib, kw

    def _set(self, values):
        for k, v in values.items():
            self.lib.cv_lm1_set_option(_handle(self.lib), k.encode(), i32(v))

    def __enter__(self):
        self._set(self.kw)

    def __exit__(self, *exc):
        self._set({k: 1 for k in self.kw})


def _run_gemv(lib, form, N, K, seed=0, **kw):
    q = Gemv(N, K, 7 * N + K + seed, **kw)
    assert _form(N, K, q.bf16, q.pro) == form, (_form(N, K, q.bf16, q.pro), form)
    y = q.launch(lib)
    q.check(y, form, "%s N=%d K=%d" % (form, N, K))
    if q.kp > K:                                                # the pad columns K .. kp - 1 are multiplied by zeros of xs: 3e4 or 0 there, the same bits
        assert torch.equal(Gemv(N, K, 7 * N + K + seed, pad=3.0e4, **kw).launch(lib), y), "the pad columns of W changed the result"
    return q, y


# (form, N, K): the smallest shapes that reach each form and each of its edges
_F32 = [("gemv<4,4,f32>", N, K) for K in (4, 36, 64, 100, 1020, 1024) for N in (1, 3, 5, 130)]
_F32 += [("gemv16<f32,16,1,4,whole>", N, K) for K in (64, 512, 1024) for N in (2048, 2050)]
_F32 += [("gemv<4,4,f32>", 2048, 96)]                           # kp = 96 is no multiple of 64: the whole-row form falls back to the narrow one
_F32 += [("gemv<8,8,f32>", N, K) for K in (1028, 1280, 4092, 4096) for N in (5, 1024)]
_F32 += [("gemv<8,4,f32>", 2052, 1088), ("gemv<8,4,f32>", 2052, 2112)]          # the form no model reaches; K = 2112: 33 steps, the last wave's share is 9 of the 16 steps a lane holds
_BF16 = [("gemv16<bf16,8,1,4,whole>", N, K) for K in (128, 1024) for N in (2048, 2050)]
_BF16 += [("gemv16<bf16,2,1,4,ksplit>", N, K) for K in (128, 640, 1024) for N in (3, 130)]      # K = 128: three waves with no step; 640: shares 1, 1, 1, 2
_BF16 += [("gemv16<bf16,4,1,8,ksplit>", 5, 1152), ("gemv16<bf16,4,1,8,ksplit>", 5, 4096), ("gemv16<bf16,4,1,8,ksplit>", 130, 1152)]        # st = 9: shares 1 x 7, 2
_BF16 += [("gemv<4,4,bf16>", N, K) for K in (64, 96, 192) for N in (3, 130)]                    # kp % 128 != 0
_BF16 += [("gemv<8,8,bf16>", 5, 1056), ("gemv<8,4,bf16>", 2052, 1056)]


def _slow(N, K):
    return N >= 2048 and K >= 1024


def _ids(rows):
    return ["%s-N%d-K%d" % r for r in rows]


@pytest.mark.parametrize("form,N,K", _F32, ids=_ids(_F32))
def test_gemv_fp32_forms(lib, form, N, K):
    _run_gemv(lib, form, N, K)


@pytest.mark.parametrize("form,N,K", _BF16, ids=_ids(_BF16))
def test_gemv_bf16_forms(lib, form, N, K):
    _run_gemv(lib, form, N, K, bf16=True)


@pytest.mark.parametrize("N", [1, 3, 5, 130])
def test_gemv_rows_per_group_give_the_same_bits(lib, N):
    """gemv_rows / gemv_rows16 = 1, 2, 4 with N no multiple of 4 rows: the clamped rows of the last workgroup, the same bits across the three, fp32 and bf16."""
    for bf16, opt, K in ((False, "gemv_rows", 100), (True, "gemv_rows16", 96), (False, "gemv_rows", 1280)):
        q = Gemv(N, K, 300 + N, bf16=bf16)
        form = _form(N, K, bf16, NONE)
        ops = q.device(lib)
        ys = []
        for rows in (1, 2, 4):
            with _options(lib, **{opt: rows}):
                ys.append(q.launch(lib, ops))
        q.check(ys[0], form, "rows N=%d K=%d" % (N, K))
        assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])


def test_gemv_rows_per_group_under_a_prologue(lib):
    """gemv_rows / gemv_rows16 = 1, 2, 4 behind the LayerNorm and the merge prologue (the lane that finishes a row changes with the rows per group, the vector in
    LDS does not): the same bits across the three, rows = 1 inside the float64 bound, nothing written behind y (launch)."""
    for bf16, opt, N, K, pro in ((False, "gemv_rows", 5, 100, LN), (False, "gemv_rows", 130, 64, MERGE), (True, "gemv_rows16", 5, 96, LN), (True, "gemv_rows16", 130, 64, MERGE)):
        q = Gemv(N, K, 1000 + N + K, bf16=bf16, pro=pro)
        narrow = {"gemv16_wide": 0} if bf16 else {}
        form = _form(N, K, bf16, pro, wide16=0 if bf16 else 1)
        assert form.startswith("gemv<")
        ops = q.device(lib)
        ys = []
        for rows in (1, 2, 4):
            with _options(lib, **{opt: rows}, **narrow):
                ys.append(q.launch(lib, ops))
        q.check(ys[0], form, "rows pro=%d N=%d K=%d" % (pro, N, K))
        assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2]), "pro=%d N=%d K=%d bf16=%s: the rows per group changed the bits" % (pro, N, K, bf16)


def test_gemv_wide_options_off(lib):
    """gemv_wide = 0 at K = 512 and gemv16_wide = 0 at K = 1024 / 1280: the narrow forms on shapes the whole-row / K-split forms serve by default.  The bits may differ;
    both forms are inside the bound."""
    for bf16, opt, N, K in ((False, "gemv_wide", 2050, 512), (True, "gemv16_wide", 130, 1024), (True, "gemv16_wide", 5, 1280)):
        q = Gemv(N, K, 400 + K, bf16=bf16)
        ops = q.device(lib)
        q.check(q.launch(lib, ops), _form(N, K, bf16, NONE), "default N=%d K=%d" % (N, K))
        with _options(lib, **{opt: 0}):
            narrow = _form(N, K, bf16, NONE, wide=0, wide16=0)
            assert narrow.startswith("gemv<")
            q.check(q.launch(lib, ops), narrow, "%s=0 N=%d K=%d" % (opt, N, K))


_LN = [(N, K, eps) for K, N in ((64, 5), (100, 130), (512, 3), (1020, 5), (1024, 130)) for eps in (1e-12, 1e-5)] + [(2050, 512, 1e-5)]


@pytest.mark.parametrize("N,K,eps", _LN)
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_gemv_layernorm_prologue(lib, N, K, eps, bf16):
    """The LayerNorm prologue at K = 64, 100, 512, 1020, 1024 (every wave parks its chunk; K % 256 != 0 and K < 256 leave waves without one), both eps of the model."""
    form = _form(N, K, bf16, LN)
    q = Gemv(N, K, 500 + K + N, bf16=bf16, pro=LN, eps=eps)
    y = q.launch(lib)
    q.check(y, form, "LN %s N=%d K=%d eps=%g" % (form, N, K, eps))
    if q.kp > K:
        assert torch.equal(Gemv(N, K, 500 + K + N, bf16=bf16, pro=LN, eps=eps, pad=3.0e4).launch(lib), y)


@pytest.mark.parametrize("K", [100, 1024])
def test_gemv_layernorm_of_a_stiff_row(lib, K):
    """A row with mean 100 and spread 0.1: the centred values keep ~10 bits.  The bound carries the fp32 mean's error through (the smallest product does not
    stand out of it here: that premise belongs to the well-conditioned rows above)."""
    q = Gemv(5, K, 600 + K, pro=LN, eps=1e-12, stiff=True)
    q.check(q.launch(lib), _form(5, K, False, LN), "stiff LN K=%d" % K, significant=False)


@pytest.mark.parametrize("K", [64, 128, 1024])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_gemv_merge_prologue(lib, K, bf16):
    """The MERGE prologue on crafted partials: empty ranges (-inf, 0, 0), maxima 95 apart inside a head, a head whose last two ranges are empty."""
    N = 130
    form = _form(N, K, bf16, MERGE)
    q = Gemv(N, K, 700 + K, bf16=bf16, pro=MERGE)
    q.check(q.launch(lib), form, "MERGE %s K=%d" % (form, K))


@pytest.mark.parametrize("act", ["none", "relu", "silu"])
@pytest.mark.parametrize("bias,res", [(True, True), (True, False), (False, True), (False, False)], ids=["bias-res", "bias", "res", "plain"])
def test_gemv_epilogue(lib, act, bias, res):
    for bf16, N, K in ((False, 130, 100), (True, 130, 640), (False, 2050, 64)):
        q = Gemv(N, K, 800 + K, bf16=bf16, act=act, bias=bias, res=res)
        q.check(q.launch(lib), _form(N, K, bf16, NONE), "act=%s bias=%s res=%s N=%d K=%d" % (act, bias, res, N, K))


# ---- the batched twins ---------------------------------------------------------------------------------------------------------------------------------------

def _masks(nb):
    out = {(1 << nb) - 1, 1, 1 << (nb - 1), sum(1 << i for i in range(0, nb, 2))}
    return sorted(out)


def _batch_launch(lib, qs, nb, mask, o):
    """cv_lm1_gemv_batch on the vectors of qs (one Gemv per slot, sharing W / bias / gamma / beta).  x and res hold the ACTIVE slots' rows only up to the last active
    one - an inactive slot in between holds NaN, the slots behind lie past the end of the allocation (the contract: no pointer of an inactive slot is read)."""
    q0 = qs[0]
    last = max(i for i in range(nb) if mask >> i & 1)
    xs = torch.stack([qs[i].x if mask >> i & 1 else torch.full_like(q0.x, float("nan")) for i in range(last + 1)])
    rs = None if q0.res is None else torch.stack([qs[i].res if mask >> i & 1 else torch.full_like(q0.res, float("nan")) for i in range(last + 1)])
    xs, rs = _dev(lib, xs), _dev(lib, rs)
    sy = q0.N + TAIL
    y = _dev(lib, _sent(nb * sy))
    h = _handle(lib)
    lib.cv_lm1_batch_begin(h, i32(nb), stream_ptr(lib))
    lib.cv_lm1_gemv_batch(h, i32(nb), u32(mask), i32(q0.pro), _p(xs), i64(q0.x.numel()), _p(o["g"]), _p(o["b"]), f32(q0.eps), _p(None if q0.bf16 else o["W"]),
                          _p(o["W"] if q0.bf16 else None), _p(o["bias"]), _p(rs), i64(q0.N), _p(y), i64(sy), i32(q0.N), i32(q0.K), i32(ACT[q0.act]), stream_ptr(lib))
    _sync(lib)
    return y.cpu().clone().reshape(nb, sy)


# a representative shape of every form (and prologue): (N, K, bf16, pro)
_TWINS = [(5, 100, False, NONE), (130, 1024, False, LN), (2050, 64, False, NONE), (5, 4092, False, NONE), (2052, 1088, False, NONE),
          (2050, 128, True, LN), (3, 640, True, NONE), (130, 128, True, MERGE), (5, 1152, True, NONE), (5, 4096, True, NONE), (3, 96, True, NONE), (5, 1056, True, NONE),
          (2052, 1056, True, NONE), (130, 64, False, MERGE)]


@pytest.mark.parametrize("N,K,bf16,pro", _TWINS, ids=["%s-N%d-K%d-pro%d" % (_form(N, K, b, p), N, K, p) for N, K, b, p in _TWINS])
def test_gemv_batched_twins(lib, N, K, bf16, pro):
    """nb = 1, 2, 3, 5, 8 slots; all active, one active (the first, the last), alternating: every active slot has the bits of cv_lm1_gemv on its vector alone, every
    inactive slot's y keeps the sentinel, nothing is written behind a slot's N elements.  The K > 1024 shapes stage two slots per pass: 1, 1, 2, 3 and 4 passes."""
    qs = [Gemv(N, K, 900 + K, bf16=bf16, pro=pro, act="relu" if pro == LN else "none") for _ in range(8)]
    g = _gen(K + N)
    for i, q in enumerate(qs[1:], 1):                            # the slots share the matrix, bias, gamma and beta; x and res are their own
        q.W, q.bias, q.g, q.b = qs[0].W, qs[0].bias, qs[0].g, qs[0].b
        q.x = (q.x[torch.randperm(q.x.numel(), generator=g)] if pro != MERGE else Gemv(N, K, 900 + K + i, bf16=bf16, pro=pro).x)
        q.res = _mag((N,), g)
    ops = qs[0].device(lib)
    alone = []
    for q in qs:
        o = dict(ops, x=_dev(lib, q.x), res=_dev(lib, q.res))
        alone.append(q.launch(lib, o))
    qs[0].check(alone[0], _form(N, K, bf16, pro), "slot vector alone")
    for nb in (1, 2, 3, 5, 8):
        if lib.emulated and N >= 2048 and nb in (2, 5):
            continue                                             # (emulator time: the whole-row shapes keep nb = 1, 3, 8)
        for mask in _masks(nb):
            y = _batch_launch(lib, qs, nb, mask, ops)
            for i in range(nb):
                if mask >> i & 1:
                    assert torch.equal(y[i, :N], alone[i]), "nb=%d mask=%x: slot %d differs from cv_lm1_gemv on its vector" % (nb, mask, i)
                    assert bool((y[i, N:] == _S32).all())
                else:
                    assert bool((y[i] == _S32).all()), "nb=%d mask=%x: inactive slot %d was written" % (nb, mask, i)


# ---- argument checks -----------------------------------------------------------------------------------------------------------------------------------------

def test_attention_arguments_are_checked(lib):
    """One accepted call, then each refused argument: an error that names the hook, nothing launched (`part` keeps the sentinel)."""
    c = _random_case(9, 1, 3)
    rows, tab = _dev(lib, c.rows), _dev(lib, c.tab)
    part = _dev(lib, _sent(3 * 8 * 66))
    good = dict(nb=0, rows=[rows.data_ptr()] * 3, tabs=[tab.data_ptr()] * 3, n_tab=[9, 9, 9], pos=[8, 8, 8], d=64, heads=1, scale=SCALE, part=part.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        lib.cv_lm1_attention(i32(a["nb"]), (C.c_void_p * 9)(*a["rows"]), (C.c_void_p * 9)(*a["tabs"]), (i32 * 9)(*a["n_tab"]), (i32 * 9)(*a["pos"]), i32(a["d"]), i32(a["heads"]),
                             f32(a["scale"]), C.c_void_p(a["part"]), stream_ptr(lib))
        _sync(lib)

    bad = [dict(rows=[None] * 3), dict(tabs=[None] * 3), dict(rows=[rows.data_ptr() + 4] * 3), dict(tabs=[tab.data_ptr() + 8] * 3), dict(part=None),
           dict(d=128), dict(d=64 * 17, heads=17), dict(heads=0, d=0), dict(pos=[32768] * 3, n_tab=[40000] * 3), dict(n_tab=[8] * 3), dict(nb=9), dict(nb=-1),
           dict(scale=0.0), dict(scale=-0.125), dict(scale=float("inf")), dict(scale=float("nan")),
           dict(nb=3, rows=[rows.data_ptr(), None, None], pos=[8, -1, 8]),                                      # a null pointer of an ACTIVE slot (slot 2)
           dict(nb=2, n_tab=[9, 8])]
    for kw in bad:
        with pytest.raises(CosyVoiceAmdError, match="cv_lm1_attention"):
            call(**kw)
    assert bool((part.cpu() == _S32).all()), "a refused call launched"
    call()
    call(nb=3, rows=[rows.data_ptr(), None, rows.data_ptr()], tabs=[tab.data_ptr(), None, tab.data_ptr()], pos=[8, -1, 8])


def test_gemv_arguments_are_checked(lib):
    keep = []
    h, h32 = _handle(lib), _make_handle(lib, keep)
    N, K = 5, 64
    x, W, y = _dev(lib, torch.zeros(2 * K + 4)), _dev(lib, torch.zeros(N * K + 4)), _dev(lib, _sent(8 * (N + TAIL)))
    W16 = _dev(lib, torch.zeros(N * K + 8, dtype=torch.bfloat16))
    gb = _dev(lib, torch.ones(K + 4))
    part = _dev(lib, torch.zeros(8 * 66))
    good = dict(m=h, pro=NONE, x=x.data_ptr(), g=None, b=None, eps=1e-5, W=W.data_ptr(), W16=None, bias=None, res=None, y=y.data_ptr(), N=N, K=K, act=ACT["none"],
                nb=2, mask=3, sx=K, sres=N, sy=N + TAIL)

    def single(**kw):
        a = dict(good, **kw)
        lib.cv_lm1_gemv(a["m"], i32(a["pro"]), C.c_void_p(a["x"]), C.c_void_p(a["g"]), C.c_void_p(a["b"]), f32(a["eps"]), C.c_void_p(a["W"]), C.c_void_p(a["W16"]),
                        C.c_void_p(a["bias"]), C.c_void_p(a["res"]), C.c_void_p(a["y"]), i32(a["N"]), i32(a["K"]), i32(a["act"]), stream_ptr(lib))
        _sync(lib)

    def batch(**kw):
        a = dict(good, **kw)
        lib.cv_lm1_gemv_batch(a["m"], i32(a["nb"]), u32(a["mask"]), i32(a["pro"]), C.c_void_p(a["x"]), i64(a["sx"]), C.c_void_p(a["g"]), C.c_void_p(a["b"]), f32(a["eps"]),
                              C.c_void_p(a["W"]), C.c_void_p(a["W16"]), C.c_void_p(a["bias"]), C.c_void_p(a["res"]), i64(a["sres"]), C.c_void_p(a["y"]), i64(a["sy"]),
                              i32(a["N"]), i32(a["K"]), i32(a["act"]), stream_ptr(lib))
        _sync(lib)

    bad = [dict(m=None), dict(pro=3), dict(pro=-1), dict(x=None), dict(y=None), dict(x=x.data_ptr() + 4), dict(y=y.data_ptr() + 2), dict(W=None), dict(W16=W16.data_ptr()),
           dict(W=W.data_ptr() + 4), dict(W=None, W16=W16.data_ptr() + 2), dict(m=h32, W=None, W16=W16.data_ptr()), dict(N=0), dict(K=0), dict(K=62), dict(K=4100),
           dict(pro=LN), dict(pro=LN, g=gb.data_ptr(), b=gb.data_ptr() + 4), dict(pro=LN, g=gb.data_ptr(), b=gb.data_ptr(), eps=float("nan")),
           dict(pro=LN, g=gb.data_ptr(), b=gb.data_ptr(), eps=-1.0), dict(pro=LN, g=gb.data_ptr(), b=gb.data_ptr(), K=1028), dict(pro=MERGE, x=part.data_ptr(), K=32),
           dict(pro=MERGE, x=part.data_ptr(), K=1088), dict(act=ACT["gelu_erf"]), dict(act=-1), dict(bias=x.data_ptr() + 2), dict(res=x.data_ptr() + 1)]
    try:
        for kw in bad:
            with pytest.raises(CosyVoiceAmdError, match="cv_lm1_gemv:"):
                single(**kw)
        with pytest.raises(CosyVoiceAmdError, match="cv_lm1_gemv_batch"):
            batch(m=h32)                                         # no cv_lm1_batch_begin on that handle yet
        lib.cv_lm1_batch_begin(h, i32(2), stream_ptr(lib))
        for kw in bad + [dict(nb=3), dict(nb=0), dict(nb=9), dict(mask=4), dict(sx=K + 2), dict(sx=-K), dict(sres=-1), dict(sy=-1)]:
            with pytest.raises(CosyVoiceAmdError, match="cv_lm1_gemv_batch"):
                batch(**kw)
        assert bool((y.cpu() == _S32).all()), "a refused call launched"
        single()
        single(W=None, W16=W16.data_ptr())
        single(pro=LN, g=gb.data_ptr(), b=gb.data_ptr())
        single(pro=MERGE, x=part.data_ptr())
        batch()
        batch(mask=0)
        batch(mask=2, x=x.data_ptr() - 4 * K)                    # slot 0 is inactive: its pointers are never formed into a load
    finally:
        lib.raw("cv_lm1_destroy", None)(h32)


def test_gemv_batch_refuses_a_handle_with_an_open_slot(emu_lib):
    """cv_lm1_gemv_batch owns the slot flags for the length of the call: a handle with a request in a slot is refused, and afterwards the flags are clear again (a batched
    GEMV with every slot's bit clear writes nothing - checked through a second call with mask 0 above; here: the refusal)."""
    from cosyvoice_amd.llm import SamplingC
    lib, keep = emu_lib, []
    h = _make_handle(lib, keep)
    try:
        d = 64
        rows, tabs, x, emb = torch.zeros(8, 4 * d), torch.zeros(15, d), torch.zeros(d), torch.zeros(10, d)
        pr, pt = (C.c_void_p * 1)(rows.data_ptr()), (C.c_void_p * 1)(tabs.data_ptr())
        sp = SamplingC(0, 9, 1, 0, 4, 0.8, 25, 10, 0.1, 0, 0)
        lib.cv_lm1_batch_begin(h, i32(2), None)
        lib.cv_lm1_batch_bind(h, i32(1), pr, pt, i32(8), i32(8), None)
        lib.cv_lm1_batch_open(h, i32(1), _p(x), i32(0), C.byref(sp), _p(emb), i32(4), None, i32(0), None)
        W, y = torch.zeros(5, d), _sent(2 * 5)
        args = (h, i32(2), u32(1), i32(NONE), _p(x), i64(d), None, None, f32(0.0), _p(W), None, None, None, i64(0), _p(y), i64(5), i32(5), i32(d), i32(0), None)
        with pytest.raises(CosyVoiceAmdError, match="cv_lm1_gemv_batch: the handle has an open slot"):
            lib.cv_lm1_gemv_batch(*args)
        assert bool((y == _S32).all())
        lib.cv_lm1_batch_release(h, i32(1))
        lib.cv_lm1_gemv_batch(*args)
        assert bool((y[:5] == 0).all()) and bool((y[5:] == _S32).all())
    finally:
        lib.raw("cv_lm1_destroy", None)(h)


def test_gemv_batch_ignores_a_stale_flag_beyond_its_slots(emu_lib):
    """cv_lm1_batch_begin(3) on a handle whose slot 3 of an earlier batch of 8 was left open: that slot's device flag is still set, and the kernels instantiated for
    4 slots must not finish it (lane `sub` of a group finishes slot `sub` only below nb)."""
    from cosyvoice_amd.llm import SamplingC
    lib, keep = emu_lib, []
    h = _make_handle(lib, keep)
    try:
        d, N = 64, 5
        rows, tabs, emb = torch.zeros(8, 4 * d), torch.zeros(15, d), torch.zeros(10, d)
        pr, pt = (C.c_void_p * 1)(rows.data_ptr()), (C.c_void_p * 1)(tabs.data_ptr())
        sp = SamplingC(0, 9, 1, 0, 4, 0.8, 25, 10, 0.1, 0, 0)
        x = torch.ones(4, d)
        lib.cv_lm1_batch_begin(h, i32(8), None)
        lib.cv_lm1_batch_bind(h, i32(3), pr, pt, i32(8), i32(8), None)
        lib.cv_lm1_batch_open(h, i32(3), _p(x), i32(0), C.byref(sp), _p(emb), i32(4), None, i32(0), None)
        lib.cv_lm1_batch_begin(h, i32(3), None)
        W, y = torch.ones(N, d), _sent(4 * N)
        lib.cv_lm1_gemv_batch(h, i32(3), u32(7), i32(NONE), _p(x), i64(d), None, None, f32(0.0), _p(W), None, None, None, i64(0), _p(y), i64(N), i32(N), i32(d), i32(0), None)
        assert bool((y[:3 * N] == 64.0).all()) and bool((y[3 * N:] == _S32).all())
    finally:
        lib.raw("cv_lm1_destroy", None)(h)
