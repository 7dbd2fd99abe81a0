"""The per-forward weight preparation kernels of the WaveGlow forward, one by one through the C entry points, against float64:

  t2s_wg_endfold_weights    F = (W_end . diag(scale)) . V_skip per layer, scattered into the gate epilogue's A fragments
                            (fold_A: [mt][wr][pair][hi, lo][lane = q * 16 + r][element half * 4 + reg]), and bes = W_end . b_skip
  t2s_wg_startfold_weights  (g / |v|) v[:, :, tap] . [W_start | b_start] as the first nwc K-chunks of a gate A operand
                            ([K-chunk][Mpad][32], T2S_PERM_GATE rows, four column sets)

The shapes are the smallest at which the tiling can go wrong: endfold's workgroup is (layer, 32 columns) with 32 slices of the
o reduction in chunks of 256 rows (C = 32: one block, one row per slice; 48: a partial column block; 160: slices and a chunk that
are partial; 512: two chunks); startfold's wave stages one row and halves its C range (C = 50: the unvectorised staging).
Bars are tests/wg_bwd_util.py's: plane outputs at GEMM_*, f32 small operations at F32_*."""
import pytest
import torch

import wg_bwd_util as U
from wg_fwd_util import _endfold_decode, _gate_row
from text2speech_amd import _lib, planes

pytestmark = pytest.mark.gpu

DEV = U.DEV
PAD = 1024          # bf16 elements in front of and behind every plane output


class _Planes:
    """A zeroed bf16 device buffer of n elements with PAD elements either side; `.t` is the buffer."""

    def __init__(self, n):
        self.n = n
        self.raw = torch.zeros(n + 2 * PAD, dtype=torch.bfloat16, device=DEV)
        self.t = self.raw[PAD:PAD + n]

    def assert_guards(self, label):
        assert float(self.raw[:PAD].float().abs().max()) == 0.0, "%s: wrote in front of the output" % label
        assert float(self.raw[PAD + self.n:].float().abs().max()) == 0.0, "%s: wrote behind the output" % label


# ---------------------------------------------------------------------------------------------- endfold
def _endfold_inputs(C, specs, seed):
    """specs: (nj, with_scale) per job -> the jobs' tensors, seeded"""
    gen = torch.Generator().manual_seed(seed)
    jobs = []
    for nj, with_scale in specs:
        jobs.append(dict(nj=nj,
                         w_end=U.dev(torch.randn(nj, C, generator=gen) * 0.05),
                         v=U.dev(torch.randn(C, C, generator=gen)),
                         scale=U.dev(torch.rand(C, generator=gen) + 0.5) if with_scale else None,
                         b=U.dev(torch.randn(C, generator=gen))))
    return jobs


def _endfold_run(C, jobs):
    for j in jobs:
        j["fold"] = _Planes(-(-C // 128) * 8192)
        j["bes"] = U.Guarded(8)
    ptr = lambda t: 0 if t is None else t.data_ptr()
    table = torch.tensor([[ptr(j["w_end"]), ptr(j["v"]), ptr(j["scale"]), ptr(j["b"]), ptr(j["fold"].t), ptr(j["bes"].t), j["nj"], C]
                          for j in jobs], dtype=torch.int64).to(DEV)
    _lib.call("t2s_wg_endfold_weights", _lib.ptr(table), len(jobs), C, _lib.current_stream())
    torch.cuda.synchronize()
    return table


ENDFOLD_CASES = [(32, [(8, True)]), (32, [(4, True), (6, False), (8, True)]),
                 (48, [(6, True)]),
                 (160, [(8, False)]), (160, [(4, True), (6, True), (8, True)]),
                 (512, [(8, True)]), (512, [(4, False), (6, True), (8, True)])]


@pytest.mark.parametrize("C,specs", ENDFOLD_CASES, ids=["C%d-%djobs" % (C, len(s)) for C, s in ENDFOLD_CASES])
def test_endfold_weights_vs_f64(C, specs):
    """Every job of a launch: rows r < nj of fold_A against the float64 product at the plane bar, rows nj .. 15 and the columns
    c >= C zero, nothing written outside the job's own buffers, bes for every job at the f32 bar (rows nj .. 7 zero)."""
    _lib.load()
    jobs = _endfold_inputs(C, specs, seed=C + len(specs))
    _endfold_run(C, jobs)
    for n, j in enumerate(jobs):
        label = "endfold C=%d job %d/%d nj=%d scale=%s" % (C, n, len(jobs), j["nj"], j["scale"] is not None)
        nj = j["nj"]
        ws = j["w_end"].double().cpu()
        if j["scale"] is not None:
            ws = ws * j["scale"].double().cpu()[None]
        want = ws @ j["v"].double().cpu()                      # [nj, C]
        got = _endfold_decode(j["fold"].t, C)
        U.check(label + " fold_A", got[:nj, :C], want, U.GEMM_NORM, U.GEMM_MAX)
        assert float(got[nj:].abs().max()) == 0.0, label + ": rows nj .. 15 are not zero"
        if got.size(1) > C:
            assert float(got[:, C:].abs().max()) == 0.0, label + ": columns past C are not zero"
        j["fold"].assert_guards(label)
        bes = j["bes"].t.double().cpu()
        U.check(label + " bes", bes[:nj], j["w_end"].double().cpu() @ j["b"].double().cpu(), U.F32_NORM, U.F32_MAX)
        assert float(bes[nj:].abs().max()) == 0.0 if nj < 8 else True, label + ": bes rows nj .. 7 are not zero"
        j["bes"].assert_guards(label)
    if len(jobs) > 1:       # distinct outputs: no job's result landed in another's buffer
        assert not torch.equal(jobs[0]["fold"].t, jobs[1]["fold"].t)


def test_endfold_weights_same_bits_every_launch():
    """Two launches on the same inputs (3 jobs, C = 160 and 512) give the same bits: the slices are summed in a fixed order."""
    _lib.load()
    for C in (160, 512):
        jobs = _endfold_inputs(C, [(4, True), (6, False), (8, True)], seed=7)
        _endfold_run(C, jobs)
        first = [(j["fold"].t.clone(), j["bes"].t.clone()) for j in jobs]
        _endfold_run(C, jobs)
        for j, (f, b) in zip(jobs, first):
            assert torch.equal(j["fold"].t, f) and torch.equal(j["bes"].t, b)


# ---------------------------------------------------------------------------------------------- startfold
def _startfold_inputs(C, nh, taps, with_g, seed):
    gen = torch.Generator().manual_seed(seed)
    return dict(v=U.dev(torch.randn(2 * C, C, taps, generator=gen)),
                g=U.dev(torch.rand(2 * C, generator=gen) + 0.5) if with_g else None,
                ws=U.dev(torch.randn(C, nh, generator=gen)),
                bs=U.dev(torch.randn(C, generator=gen)))


def _startfold_run(x, C, nh, taps, nwc, Mpad):
    Ah, Al = _Planes(nwc * Mpad * 32), _Planes(nwc * Mpad * 32)
    _lib.call("t2s_wg_startfold_weights", _lib.ptr(x["v"]), _lib.ptr(x["g"]), _lib.ptr(x["ws"]), _lib.ptr(x["bs"]), C, nh, taps,
              Mpad, nwc, _lib.ptr(Ah.t), _lib.ptr(Al.t), _lib.current_stream())
    torch.cuda.synchronize()
    return Ah, Al


STARTFOLD_CASES = [(64, 2, 3, True), (160, 3, 3, True), (160, 4, 3, True), (64, 4, 3, False), (64, 4, 5, True), (160, 4, 5, True),
                   (50, 4, 3, True)]


@pytest.mark.parametrize("C,nh,taps,with_g", STARTFOLD_CASES, ids=["C%d-nh%d-taps%d-%s" % (c, n, t, "g" if g else "plain")
                                                                   for c, n, t, g in STARTFOLD_CASES])
def test_startfold_weights_vs_f64(C, nh, taps, with_g):
    """The composed block against (g / |v|) v[:, :, tap] . [W_start | b_start] in float64, rows through the T2S_PERM_GATE order:
    column set 0 (the plain split pair) at the plane bar; sets 2 and 3 bit for bit (h, l) and (l, 0) of set 0; the three split
    products of every set against a window value's own four sets, recombined in float64, equal weight * window at the f32 bar;
    unused columns are zero, rows of Mpad that no channel maps to stay as the caller zeroed them, nothing outside is written."""
    _lib.load()
    ncol = taps * (nh + 1)
    nwc = 2 if 2 * ncol <= 32 else 4
    spc = 4 // nwc
    Mpad = _lib.padded_rows(2 * C)
    x = _startfold_inputs(C, nh, taps, with_g, seed=C + 10 * nh + taps)
    Ah, Al = _startfold_run(x, C, nh, taps, nwc, Mpad)
    label = "startfold C=%d nh=%d taps=%d g=%s" % (C, nh, taps, with_g)
    v = x["v"].double().cpu()
    w = U.wn_eff(v, None if x["g"] is None else x["g"].double().cpu())
    wb = torch.cat([x["ws"].double().cpu(), x["bs"].double().cpu()[:, None]], 1)
    want = torch.einsum("mct,cj->mtj", w, wb).reshape(2 * C, ncol)
    rows = _gate_row(torch.arange(2 * C), C)
    assert int(rows.max()) < Mpad and rows.unique().numel() == 2 * C
    hi = Ah.t.view(nwc, Mpad, 32).permute(1, 0, 2).reshape(Mpad, nwc * 32).cpu()
    lo = Al.t.view(nwc, Mpad, 32).permute(1, 0, 2).reshape(Mpad, nwc * 32).cpu()
    first = [(s // spc) * 32 + (s % spc) * ncol for s in range(4)]
    sets = [(hi[rows, c0:c0 + ncol], lo[rows, c0:c0 + ncol]) for c0 in first]
    U.check(label + " set 0", sets[0][0].double() + sets[0][1].double(), want, U.GEMM_NORM, U.GEMM_MAX)
    assert torch.equal(sets[2][0], sets[0][0]) and torch.equal(sets[2][1], sets[0][1]), label + ": set 2 is not set 0"
    assert torch.equal(sets[3][0], sets[0][1]) and float(sets[3][1].float().abs().max()) == 0.0, label + ": set 3 is not (l, 0)"
    # the window side of the product: one seeded f32 value per logical column, in its own four sets
    a = torch.randn(ncol, generator=torch.Generator().manual_seed(ncol))
    ah, al = planes.start_fold_sets(a, False, nwc, 0)
    rec = torch.zeros(2 * C, ncol, dtype=torch.float64)
    for s, c0 in enumerate(first):
        wh, wl = sets[s][0].double(), sets[s][1].double()
        bh, bl = ah[c0:c0 + ncol].double()[None], al[c0:c0 + ncol].double()[None]
        rec += wh * bh + wh * bl + wl * bh
    U.check(label + " four sets", rec, want * a.double()[None], U.F32_NORM, U.F32_MAX)
    used = torch.zeros(nwc * 32, dtype=torch.bool)
    for c0 in first:
        used[c0:c0 + ncol] = True
    if bool((~used).any()):
        assert float(hi[:, ~used].float().abs().max()) == 0.0 and float(lo[:, ~used].float().abs().max()) == 0.0, label
    other = torch.ones(Mpad, dtype=torch.bool)
    other[rows] = False
    if bool(other.any()):
        assert float(hi[other].float().abs().max()) == 0.0 and float(lo[other].float().abs().max()) == 0.0, \
            label + ": a row no channel maps to was written"
    Ah.assert_guards(label)
    Al.assert_guards(label)


def test_startfold_weights_same_bits_every_launch():
    """Two launches on the same inputs give the same bits (C = 160: 3 taps with two chunks, 5 taps with four)."""
    _lib.load()
    for taps, nwc in ((3, 2), (5, 4)):
        C, nh = 160, 4
        Mpad = _lib.padded_rows(2 * C)
        x = _startfold_inputs(C, nh, taps, True, seed=3)
        a = _startfold_run(x, C, nh, taps, nwc, Mpad)
        b = _startfold_run(x, C, nh, taps, nwc, Mpad)
        assert torch.equal(a[0].t, b[0].t) and torch.equal(a[1].t, b[1].t)
        assert float(a[0].t.float().abs().max()) > 0.0
