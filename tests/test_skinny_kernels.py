"""Kernel-level tests of the bf16 skinny GEMMs (cosyvoice_amd/csrc/llm_batch_kernels.h) through the cv_skinny hook, at the geometries production runs and the
tiny test models never reach: 7 k-tiles per wave, four row tiles per workgroup, the uneven 4/5/5/5 split of down's K ranges, a ragged last row tile, the second
MFMA column tile (17 .. 32 sequences) and nine row groups (the 131-row prefill).

form 0 = skinny_mfma_kernel on the row-major tensor (the reference of the bit comparisons: at most 16 sequences per call, so more rows are served in consecutive
slices of 16), form 1 = the batched decode on a fragment-ordered copy, form 2 = the prefill's walk over any number of rows on a fragment-ordered copy.

1. forms 1 and 2 equal form 0 BIT FOR BIT (same products, same k order, wave order and combine order; every column is an independent dot product);
2. slot independence: row b of a run over nb rows equals, bit for bit, the run of that row alone;
3. form 0 against a float64 product of the same bf16 weights (modes 0 and 2, no gamma).  The kernel splits an fp32 activation exactly into three bf16 terms, every
   bf16 x bf16 product is exact in fp32 and the sums are fp32, so the only errors are the roundings of the additions, each at most 2^-24 of a partial sum, and no
   partial sum exceeds S = sum_k |W[n][k] x[b][k]| over the K range (to first order).  The bound charges one such rounding per k column of the range plus four for
   the cross-wave combine:  |err| <= (K / ksplit + 4) * 2^-24 * S, plus one ulp of the result of every bias / residual addition.  (A count of one rounding per
   product TERM would be three times that; the figure is kept as the tighter of the two - the errors measured under the emulator, which does round after every
   term, stay below 1 % of it; the test prints the worst ratio of every case.)
4. nothing is written outside the valid outputs: y has one extra row and 16 extra columns of pitch, filled with a sentinel that every run checks.

Every operand goes through lib.hook (guard pages under the emulator)."""
import ctypes as C
import functools

import pytest
import torch

from cosyvoice_amd._lib import CosyVoiceAmdError

MAX_ROWS, SENTINEL, EPS = 144, -6.0e30, 1e-6

#        K  ksplit   N  rt mode gamma bias+res
CASES = [
    pytest.param((128, 1, 48, 1, 0, True, True), id="k128-one-tile-per-wave"),          # the `min(4 * lane, nt * 32 - 4)` clamp (the geometry of the model tests)
    pytest.param((160, 1, 32, 2, 0, False, False), id="k160-tiles-1-1-1-2"),
    pytest.param((896, 1, 40, 1, 0, True, True), id="k896-rt1-ragged-row-tile"),        # <1,7>, N % 16 != 0 with N % 4 == 0
    pytest.param((896, 1, 160, 4, 1, True, False), id="k896-rt4-silu-up"),              # <4,7>, the last workgroup has 2 of its 4 row tiles
    pytest.param((896, 1, 61, 2, 0, True, True), id="k896-rt2-scalar-tail"),            # <2,7>, N % 4 != 0 (forms 0 and 1; form 2 refuses it)
    pytest.param((4864, 8, 32, 2, 2, False, False), id="k4864-split8-tiles-4-5-5-5"),   # <2,5>, split-K partial layout
]
NBS = {1: (1, 5, 16, 17, 32), 2: (9, 33, 144)}     # form 2: one ragged group; three groups with a single row in the last; nine full groups
SLOTS = {1: ((32, (5, 21)), (17, (16,))), 2: ((144, (7, 140)), (33, (32,)))}       # (nb, rows checked): both column tiles / the first and the last group


@functools.lru_cache(maxsize=None)
def _inputs(case):
    K, ksplit, N, rt, mode, gamma, addends = case
    g = torch.Generator().manual_seed(K + N + rt)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    x = torch.randn(MAX_ROWS, K, generator=g) * 1.7
    gam = 1 + 0.1 * torch.randn(K, generator=g) if gamma else None
    bias = torch.randn(N, generator=g) * 0.1 if addends else None
    res = torch.randn(MAX_ROWS, N, generator=g) if addends else None
    return dict(w=w, x=x, gamma=gam, bias=bias, res=res)


_dev, _runs = {}, {}


def _operand(lib, case, name, r0=None, r1=None):
    """One operand on the library's device, made once (rows [r0, r1) of the per-row ones)."""
    key = (id(lib), case, name, r0, r1)
    if key not in _dev:
        t = _inputs(case)[name]
        if t is not None and r0 is not None:
            t = t[r0:r1]
        _dev[key] = None if t is None else lib.hook(t.to(lib.device).contiguous())
    return _dev[key]


def _run(lib, case, form, r0, r1, gamma=True):
    """Rows [r0, r1) of the case's activations through one form: [ksplit or 1][rows][outputs per row], computed once and shared (read-only)."""
    key = (id(lib), case, form, r0, r1, gamma)
    if key in _runs:
        return _runs[key]
    K, ksplit, N, rt, mode, _, _ = case
    nb, n_out, parts = r1 - r0, (N // 2 if mode == 1 else N), (ksplit if mode == 2 else 1)
    pitch = n_out + 16
    y = lib.hook(torch.full((parts * nb + 1, pitch), SENTINEL, device=lib.device))
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    gam = _operand(lib, case, "gamma") if gamma else None
    lib.cv_skinny(p(_operand(lib, case, "w")), p(_operand(lib, case, "bias")), p(_operand(lib, case, "x", r0, r1)), C.c_int64(K), p(y), C.c_int64(pitch),
                  C.c_int32(N), C.c_int32(K), p(gam), C.c_float(EPS), p(_operand(lib, case, "res", r0, r1)), C.c_int64(N), C.c_int32(mode), C.c_int32(nb),
                  C.c_int32(ksplit), C.c_int32(2 if form == 0 and rt == 4 else rt),      # the row-major ladder has no four-tile form; rt does not enter the arithmetic
                  C.c_int32(form), None)
    out = y.cpu()
    assert bool((out[-1] == SENTINEL).all()) and bool((out[:, n_out:] == SENTINEL).all()), "written outside the valid outputs"
    assert bool((out[:-1, :n_out] != SENTINEL).all()), "a valid output was not written"
    _runs[key] = out[:-1, :n_out].reshape(parts, nb, n_out).clone()
    return _runs[key]


def _row_major(lib, case, nb):
    """form 0 over nb rows: consecutive slices of 16, the per-slice outputs ([ksplit][16][N] in mode 2) put together row by row."""
    return torch.cat([_run(lib, case, 0, r, min(r + 16, nb)) for r in range(0, nb, 16)], dim=1)


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("case", CASES)
def test_fragment_ordered_forms_equal_the_row_major_kernel_bit_for_bit(lib, case, form):
    for nb in NBS[form]:
        if form == 2 and case[2] % 4 != 0:                       # the rows walk has no scalar tail: an error, not a launch
            with pytest.raises(CosyVoiceAmdError, match="cv_skinny"):
                _run(lib, case, form, 0, nb)
            continue
        got, want = _run(lib, case, form, 0, nb), _row_major(lib, case, nb)
        assert got.shape == want.shape
        assert torch.equal(got, want), (nb, int((got != want).sum()), float((got - want).abs().max()))


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("case", CASES)
def test_a_row_does_not_depend_on_its_slot_or_on_the_other_rows(lib, case, form):
    if form == 2 and case[2] % 4 != 0:
        return                                                   # refused (asserted above)
    for nb, rows in SLOTS[form]:
        full = _run(lib, case, form, 0, nb)
        for b in rows:
            alone = _run(lib, case, form, b, b + 1)
            assert torch.equal(full[:, b], alone[:, 0]), (nb, b, float((full[:, b] - alone[:, 0]).abs().max()))


def _ulp32(v):
    """One unit in the last place of the fp32 number nearest to v (float64 tensor)."""
    return torch.ldexp(torch.ones_like(v), torch.frexp(v.float().double())[1] - 24)


@pytest.mark.parametrize("case", [c for c in CASES if c.values[0][4] in (0, 2)])
def test_row_major_kernel_against_float64(lib, case):
    K, ksplit, N, rt, mode, _, _ = case
    nb, step = 16, K // ksplit
    inp = _inputs(case)
    got = _run(lib, case, 0, 0, nb, gamma=False).double()
    w, x = inp["w"].double(), inp["x"][:nb].double()
    worst = 0.0
    for s in range(ksplit):
        ws, xs = w[:, s * step:(s + 1) * step], x[:, s * step:(s + 1) * step]
        want = xs @ ws.T
        bound = (step + 4) * 2.0 ** -24 * (xs.abs() @ ws.abs().T)
        if inp["bias"] is not None:
            want = want + inp["bias"].double()
            bound = bound + _ulp32(want)
            want = want + inp["res"][:nb].double()
            bound = bound + _ulp32(want)
        err = (got[s] - want).abs()
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all()), (s, float((err / bound).max()))
    print("skinny_mfma_kernel %s: worst |err| / bound = %.3g" % (case, worst))
