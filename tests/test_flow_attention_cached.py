"""The attention of the incremental flow pass (attn_cached_kernel + attn_cached_merge_kernel, csrc/flow_attn_cached.h) against a float64 reference, through its test
entry point cv_flow_attention_cached - the production grid and instantiations of cv_flow_stream_chunk.  Tn new queries at absolute positions q0 .. q0 + Tn - 1 of
every batch row attend the row's own cache: query i sees keys < min(klen[b], ((q0 + i) / chunk + 1) chunk).

Reference: the operands as the kernel takes them (fp32, or rounded to bf16 first); scores, mask, softmax and P.V in float64.  Every operand is allocated at its exact
size through lib.hook: under the emulator it ends flush against an inaccessible page, so a read of a cache row at or beyond klen[b] faults.

Tolerances (derived, not tuned), with vmax = max |v| over the keys a query sees and u = 2^-24:
  bf16 form  |o - ref| <= 2^-8 (vmax + |ref|) (1 + 2^-5): P is rounded to bf16 before P.V while the denominator sums the unrounded P (2^-8 vmax), the output is rounded to
             bf16 (2^-8 |o|), 2^-5 covers the fp32 score / exp2 / denominator / merge roundings - the bound of tests/test_flow_attention.py for the same rounding points.
  fp32 form  |o - ref| <= u vmax (140 A + 1.07 n + 64): a score is a chain of 64 exact-product fp32 FMAs, scaled and shifted by the running maximum - |dS| <= 70 u A,
             A = scale max sum_d |q_d k_d| over the pairs of the case; a weight p_j / sum p then moves by at most 2 (|dS| + 4 u) relatively (expf to 4 u), which moves the
             output by at most that times vmax: 140 u A + 8 u.  The P.V chain adds one rounding per key and one rescale per 64-key tile (n (1 + 1/64) u), the
             denominator 18 + 3 n / 64 roundings, the division 2, the merge 3 per slice (<= 24): together <= (1.07 n + 64) u with n = the keys of the case.
With the inputs below (_case: the last key of a query's own chunk dominates, the one a chunk later would dominate it) a query that sees one key too many or too few
is off by ~0.1 .. 1 vmax."""
import ctypes as C

import pytest
import torch

from cosyvoice_amd._lib import CosyVoiceAmdError, stream_ptr

SCALE = 0.125
U = 2.0 ** -24
SENT16 = -8531                    # int16 bits of bf16 0xdead
SENT32 = float.fromhex("-0x1.5bd5bcp+62")


def _sync(lib):
    if not lib.emulated:
        torch.cuda.synchronize()


def _randn(shape, seed, std=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * std


def _case(klens, H, q0, Tn, chunk, bf16, seed):
    """q [B, Tn, H, 64] and per batch row K, V [rows, H, 64] with rows = max(klen[b], 1): near-uniform random scores plus a score bonus of 2.75 on the first key of
    every chunk (V = +1.5) and of 2.75 + 2 c on the last key of chunk c and on key klen - 1 (V = -3): the last key of a query's own chunk outweighs everything before
    it by e^2, and the one a chunk later would outweigh it by e^2."""
    B = len(klens)
    q = _randn((B, Tn, H, 64), seed, 0.5)
    q[..., 0] = 1.0
    ks, vs = [], []
    for b, n in enumerate(klens):
        n = max(n, 1)
        k = _randn((n, H, 64), seed + 10 * b + 1, 0.5); v = _randn((n, H, 64), seed + 10 * b + 2)
        j = torch.arange(n)
        c = chunk if chunk > 0 else n
        first, last = (j % c == 0), (j % c == c - 1) | (j == n - 1)
        k[first, :, 0] = 22.0; k[last, :, 0] = (22.0 + 16.0 * (j[last] // c))[:, None]
        v[first] = 1.5 + 0.1 * v[first]; v[last] = -3.0 + 0.1 * v[last]
        ks.append(k); vs.append(v)
    if bf16:
        q = q.to(torch.bfloat16).float(); ks = [k.to(torch.bfloat16).float() for k in ks]; vs = [v.to(torch.bfloat16).float() for v in vs]
    return q, ks, vs


def _launch(lib, q, ks, vs, klens, q0, chunk, slices, bf16, ldq=None, ldo=None, garbage=None):
    """-> (values [B, Tn, H, 64] float, raw output [B * Tn, ldo]).  garbage: extra rows of that value appended behind klen[b] in every cache (never to be read)."""
    B, Tn, H, _ = q.shape
    HD, dev = 64 * H, lib.device
    dt = torch.bfloat16 if bf16 else torch.float32
    ldq, ldo = ldq or HD, ldo or HD
    qt = torch.zeros(B * Tn, ldq); qt[:, :HD] = q.reshape(B * Tn, HD)
    qt = lib.hook(qt.to(dt).to(dev))
    keep, kp, vp = [qt], [], []
    for b in range(B):
        for src, ptrs in ((ks[b], kp), (vs[b], vp)):
            rows = src[:max(klens[b], 0)].reshape(-1, HD)
            if garbage is not None:
                rows = torch.cat([rows, torch.full((5, HD), garbage)])
            if rows.shape[0] == 0:
                rows = torch.zeros(1, HD)
            t = lib.hook(rows.to(dt).contiguous().to(dev))
            keep.append(t); ptrs.append(t.data_ptr())
    if bf16:
        o = lib.hook(torch.full((B * Tn, ldo), SENT16, dtype=torch.int16).view(torch.bfloat16).to(dev))
    else:
        o = lib.hook(torch.full((B * Tn, ldo), SENT32, dtype=torch.float32).to(dev))
    lib.cv_flow_attention_cached(C.c_void_p(qt.data_ptr()), C.c_int32(ldq), (C.c_void_p * B)(*kp), (C.c_void_p * B)(*vp), (C.c_int32 * B)(*klens), C.c_int32(HD),
                                 C.c_void_p(o.data_ptr()), C.c_int32(ldo), C.c_int32(B), C.c_int32(H), C.c_int32(Tn), C.c_int32(q0), C.c_int32(chunk),
                                 C.c_float(SCALE), C.c_int32(slices), C.c_int32(int(bf16)), stream_ptr(lib))
    _sync(lib)
    raw = o.cpu()
    if bf16:
        assert bool((raw.view(torch.int16)[:, HD:] == SENT16).all()) and not bool((raw.view(torch.int16)[:, :HD] == SENT16).any())
    else:
        assert bool((raw[:, HD:] == SENT32).all()) and not bool((raw[:, :HD] == SENT32).any())
    return raw[:, :HD].float().reshape(B, Tn, H, 64), raw


def _reference(q, ks, vs, klens, q0, chunk):
    """float64 -> (out [B, Tn, H, 64], vmax [B, Tn, H], A = scale max sum |q_d k_d|)."""
    B, Tn, H, _ = q.shape
    out = torch.zeros(B, Tn, H, 64, dtype=torch.float64); vmax = torch.zeros(B, Tn, H, dtype=torch.float64)
    A = 0.0
    for b in range(B):
        n = klens[b]
        if n <= 0:
            continue
        i, j = q0 + torch.arange(Tn)[:, None], torch.arange(n)[None, :]
        vis = j < (i // chunk + 1) * chunk if chunk > 0 else torch.ones(Tn, n, dtype=torch.bool)
        qd, kd, vd = q[b].double(), ks[b][:n].double(), vs[b][:n].double()
        s = torch.einsum("qhd,khd->hqk", qd, kd) * SCALE
        A = max(A, float(torch.einsum("qhd,khd->hqk", qd.abs(), kd.abs()).max()) * SCALE)
        p = torch.softmax(s.masked_fill(~vis[None], float("-inf")), -1).nan_to_num(0.0)
        out[b] = torch.einsum("hqk,khd->qhd", p, vd)
        vmax[b] = torch.where(vis[:, :, None], vd.abs().amax(-1)[None], torch.zeros((), dtype=torch.float64)).amax(1)
    return out, vmax, A


def _check(got, q, ks, vs, klens, q0, chunk, bf16, what):
    ref, vmax, A = _reference(q, ks, vs, klens, q0, chunk)
    err = (got.double() - ref).abs()
    if bf16:
        bound = 2.0 ** -8 * (vmax[..., None] + ref.abs()) * (1 + 2.0 ** -5)
    else:
        bound = (U * (140 * A + 1.07 * max(klens) + 64) * vmax)[..., None].expand_as(err)
    worst = (err - bound).flatten().argmax().item()
    assert bool((err <= bound).all()), ("%s: |o - ref| above the bound at flat index %d: err %.4g, bound %.4g, ref %.4g" %
                                        (what, worst, err.flatten()[worst].item(), bound.flatten()[worst].item(), ref.flatten()[worst].item()))
    assert chunk == 0 or float(ref.abs().max()) > 0.5               # the inputs' own property: with a chunk mask a dominant last key is in every query's sight


# key counts just below, at and above the 64-key tile edges; with 1 .. 8 slices over ceil(n / 64) tiles these are also the slice edges (one tile per slice at 2 and 3
# tiles, two at 4 tiles and 2 slices) and, where slices > tiles, empty slices
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [13, 63, 64, 65, 127, 128, 129, 192, 193, 256, 260])
def test_tile_and_slice_edges(lib, bf16, n):
    """The last two chunks of 13 positions (chunk boundaries inside a wave) as new queries against n cached keys, 2 heads, two batch rows of different cache
    lengths (n, and one key short of the first query's chunk end), every slice count 1, 2, 4, 8."""
    chunk, H = 13, 2
    Tn = 26 if n > 13 else 13
    q0 = max(0, (n + chunk - 1) // chunk * chunk - Tn)                # the last query's chunk holds key n - 1
    klens = [n, max(q0 + chunk - 1, 1)]
    q, ks, vs = _case(klens, H, q0, Tn, chunk, bf16, 100 + n)
    for slices in (1, 2, 4, 8):
        got, _ = _launch(lib, q, ks, vs, klens, q0, chunk, slices, bf16)
        _check(got, q, ks, vs, klens, q0, chunk, bf16, "n=%d slices=%d" % (n, slices))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("q0,Tn,chunk", [(0, 50, 50), (0, 100, 50), (50, 50, 50), (150, 100, 50), (0, 13, 13), (13, 26, 13), (65, 13, 13), (130, 70, 0)])
def test_query_offsets_and_chunks(lib, bf16, q0, Tn, chunk):
    """q0 in {0, one chunk, several chunks}, Tn of one and two chunks, chunk 13 and 50 (and no chunk mask), the estimator's two batch rows; padded leading dimensions of
    q and o (the estimator reads Q out of [rows][3 inner] QKV rows) are neither read as queries nor written."""
    H = 2
    klens = [q0 + Tn, q0 + Tn]
    q, ks, vs = _case(klens, H, q0, Tn, chunk, bf16, 7 + q0 + Tn)
    for slices in (1, 3):
        got, _ = _launch(lib, q, ks, vs, klens, q0, chunk, slices, bf16, ldq=3 * 64 * H, ldo=64 * H + 8)
        _check(got, q, ks, vs, klens, q0, chunk, bf16, "q0=%d Tn=%d chunk=%d slices=%d" % (q0, Tn, chunk, slices))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_rows_behind_a_cache_length_do_not_change_the_bits(lib, bf16):
    """Two batch rows with different cache lengths (one shorter than q0 + Tn, one of length 0: an all-zero output); rows appended behind klen[b] that would take all of
    the softmax if seen (K = V = 3e4) leave every output bit as it was; a query's bits do not depend on Tn (the same positions as part of a longer call)."""
    H, chunk, q0, Tn = 1, 13, 52, 26
    klens = [q0 + Tn, 60, 0]
    q, ks, vs = _case(klens, H, q0, Tn, chunk, bf16, 77)
    for slices in (1, 2):
        got, raw = _launch(lib, q, ks, vs, klens, q0, chunk, slices, bf16)
        _check(got, q, ks, vs, klens, q0, chunk, bf16, "slices=%d" % slices)
        assert float(got[2].abs().max()) == 0.0
        _, raw_g = _launch(lib, q, ks, vs, klens, q0, chunk, slices, bf16, garbage=3e4)
        assert torch.equal(raw.view(torch.int16 if bf16 else torch.int32), raw_g.view(torch.int16 if bf16 else torch.int32))
        got1, _ = _launch(lib, q[:, 13:], ks, vs, klens, q0 + 13, chunk, slices, bf16)
        assert torch.equal(got1[0], got[0, 13:])


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_an_empty_slice_merges_to_nothing(lib, bf16):
    """20 keys are one tile: with 8 slices, seven hold no key at all, and they report (m, l) = (-inf, 0) with a zero accumulator.  The merge skips them: the result
    is finite and EQUAL, bit for bit, to the one-slice result (one non-empty slice merges with weight exp(0) = 1).  130 keys are three tiles - slice 0 of 2 owns two, slice 1
    the third - and the queries of the first twelve chunks see no key of slice 1: the same (-inf, 0) case per query."""
    H, chunk = 2, 10
    for q0, Tn, n, slices in ((10, 10, 20, 8), (0, 130, 130, 2)):
        klens = [n, n]
        q, ks, vs = _case(klens, H, q0, Tn, chunk, bf16, 5 + n)
        one, _ = _launch(lib, q, ks, vs, klens, q0, chunk, 1, bf16)
        many, _ = _launch(lib, q, ks, vs, klens, q0, chunk, slices, bf16)
        assert bool(torch.isfinite(many).all())
        _check(many, q, ks, vs, klens, q0, chunk, bf16, "n=%d slices=%d" % (n, slices))
        if n == 20:
            assert torch.equal(one, many)


def test_arguments_are_checked(emu_lib):
    lib = emu_lib
    q = torch.zeros(4, 64); k = torch.zeros(8, 64); o = torch.zeros(4, 64)
    P = lambda t: C.c_void_p(t.data_ptr())

    def call(q=P(q), ldq=64, kp=k.data_ptr(), vp=k.data_ptr(), klen=8, ldc=64, o=P(o), ldo=64, B=1, H=1, Tn=4, q0=4, chunk=4, scale=SCALE, slices=1, bf16=0):
        lib.cv_flow_attention_cached(q, C.c_int32(ldq), (C.c_void_p * 1)(kp), (C.c_void_p * 1)(vp), (C.c_int32 * 1)(klen), C.c_int32(ldc), o, C.c_int32(ldo), C.c_int32(B),
                                     C.c_int32(H), C.c_int32(Tn), C.c_int32(q0), C.c_int32(chunk), C.c_float(scale), C.c_int32(slices), C.c_int32(bf16), None)
    call()
    for kw, msg in ((dict(q=None), "null operand"), (dict(B=9), "bad shape"), (dict(Tn=0), "bad shape"), (dict(q0=-1), "bad shape"), (dict(ldq=66), "bad ldq / ldc"),
                    (dict(ldc=32), "bad ldq / ldc"), (dict(ldo=62), "bad ldo"), (dict(q=C.c_void_p(q.data_ptr() + 4)), "unaligned operand"), (dict(scale=0.0), "bad scale"),
                    (dict(chunk=-1), "bad chunk"), (dict(slices=0), "bad slices"), (dict(slices=9), "bad slices"), (dict(klen=-1), "bad klen"),
                    (dict(kp=None), "null or unaligned cache base"), (dict(vp=k.data_ptr() + 4), "null or unaligned cache base")):
        with pytest.raises(CosyVoiceAmdError, match="cv_flow_attention_cached: " + msg):
            call(**kw)
