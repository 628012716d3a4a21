"""Every kernel variant of the surrogate fit (wlm_launch_fit / wlm_fit_grid in csrc/xpgnn.hip)
against the fp64 oracle, with the variant pinned, and the data and shape corners through each fit
family.  Each case asserts engine.wlm_describe -- the launcher's own decision, the record the
launch dispatches on -- before it compares numbers, so a case cannot quietly test another kernel.

Inputs, references and the case lists live in tests/fit_ref.py; tests/test_fit_cpu.py checks on
the same cases, without a GPU, that the fp64 oracle and a float32 restatement agree 4x closer than
the bars used here (weights atol 1e-4, losses rtol 1e-5, the project's existing bars), that every
fit moves, and which best-epoch rule a case gets.  The last test of the variant part checks that
the variants pinned here and the ones listed as unreachable are all the dispatcher can name."""
import numpy as np
import pytest
import torch

import fit_ref
from fit_ref import KIND, LOSS_RTOL, W_ATOL

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bikg_graph_explainability_public_amd import _lib
    _lib.load()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ("XPG_WLM", "XPG_DIAGNOSTICS", "XPG_MC_SPIN", "XPG_MC_FAULT"):
        monkeypatch.delenv(k, raising=False)


def _eng():
    from bikg_graph_explainability_public_amd import engine
    return engine


def _ids(cases):
    return [c.id for c in cases]


# ------------------------------------------------------------------ running and comparing
def _device_inputs(case):
    e = _eng()
    inp = fit_ref.inputs(case)
    bits = torch.stack([e.pack_masks(torch.as_tensor(m.copy()).to(DEV)) for m, _, _, _ in inp]).contiguous()
    y = torch.as_tensor(np.stack([y for _, y, _, _ in inp])).to(DEV)
    k = torch.as_tensor(np.stack([k for _, _, k, _ in inp])).to(DEV)
    w0 = torch.as_tensor(np.stack([w for _, _, _, w in inp])).to(DEV)
    return bits, y, k, w0


def _fit(case, monkeypatch, params=None):
    """(describe string, w [F, S], losses [F, steps], best [F]) of engine.wlm_fit under the
    case's XPG_WLM setting."""
    e = _eng()
    if case.env is not None:
        monkeypatch.setenv("XPG_WLM", case.env)
    desc = e.wlm_describe(case.F, case.R, case.S, case.B)
    bits, y, k, w0 = _device_inputs(case)
    w, losses, best, _, _ = e.wlm_fit(bits, case.S, case.B, y, k, w0, params or case.params)
    return desc, w, losses, best


def _compare(case, desc, w, losses, best):
    """Each fit of the case against its own fp64 oracle fit at the bars; prints the figures
    before it asserts."""
    w, losses, best = w.cpu().double().numpy(), losses.cpu().numpy(), best.cpu().numpy()
    ref = fit_ref.reference(case)
    ew = max(float(np.abs(w[f] - ref[f][0]).max()) for f in range(case.F))
    el = max(float(np.max(np.abs(losses[f] - ref[f][1]) / np.abs(ref[f][1]))) for f in range(case.F))
    print(f"[fit] {case.id} | {desc} | max|dw|={ew:.2e} max rel dloss={el:.2e} "
          f"best={[int(b) for b in best]} oracle={[r[2] for r in ref]}")
    for f in range(case.F):
        rw, rl, rb = ref[f]
        np.testing.assert_allclose(w[f], rw, rtol=0, atol=W_ATOL, err_msg=f"{case.id} fit {f}")
        np.testing.assert_allclose(losses[f], rl, rtol=LOSS_RTOL, atol=0, err_msg=f"{case.id} fit {f}")
        rule, allowed = fit_ref.best_epochs(rl)
        assert int(best[f]) in allowed, (case.id, f, rule, int(best[f]), allowed)
        if rule == "strict":
            assert int(best[f]) == rb


def _prepared(case):
    """(w, losses, best) of PreparedFit.prepare + fit on the case's inputs."""
    e = _eng()
    bits, y, k, w0 = _device_inputs(case)
    pf = e.PreparedFit(case.F, case.R, case.S, case.B, case.params, DEV)
    pf.prepare(bits, y, k, w0)
    w = pf.fit(bits, k)
    e.check_fit_status(pf.status)
    return w, pf.losses, pf.best


# ------------------------------------------------------------------ every variant, pinned
# (XPG_WLM, F, R, S, B) -> the describe string on the MI355X (256 CUs, 8 XCDs); the shapes are
# fit_ref.VARIANT_SHAPES
TABLE = {
    ("single", 1, 128, 100, 32): "single<CPT=1,stage> n_bs=4 n_ds=1",
    ("single", 1, 128, 1025, 32): "single<CPT=2,stage> n_bs=11 n_ds=1",
    ("single", 1, 128, 2049, 32): "single<CPT=4,stage> n_bs=13 n_ds=1",
    ("single", 1, 128, 4097, 32): "single<CPT=8,stage> n_bs=15 n_ds=1",
    ("single", 1, 1760, 1000, 352): "single<CPT=1,nostage> n_bs=8 n_ds=1",
    ("single", 1, 1024, 1500, 256): "single<CPT=2,nostage> n_bs=4 n_ds=2",
    ("single", 1, 132, 4096, 33): "single<CPT=4,nostage> n_bs=16 n_ds=1",
    ("single", 1, 128, 6144, 32): "single<CPT=8,nostage> n_bs=16 n_ds=1",
    ("single", 1, 128, 8193, 32): "single<CPT=16,nostage> n_bs=16 n_ds=1",
    ("mc", 1, 128, 100, 32): "multi<C=1,G=1> P=2 wpp=2 ds=1",
    ("mc", 1, 1408, 128, 352): "multi<C=1,G=2> P=2 wpp=2 ds=8",
    ("mc", 1, 1600, 200, 400): "multi<C=1,G=4> P=3 wpp=3 ds=8",
    (None, 1, 640, 4608, 160): "multi<C=2,G=2> P=16 wpp=9 ds=4",
    (None, 1, 864, 2560, 288): "multi<C=2,G=4> P=16 wpp=5 ds=8",
    (None, 33, 96, 12450, 32): "multi<C=4,G=4> P=6 wpp=65 ds=1",
    ("grid3", 1, 128, 100, 32): "grid3 n_wg=1",
    ("grid", 1, 128, 100, 32): "grid_fused ch=1 nwg=1 nrbp=4",
}

# Instantiations no shape reaches, with the planner's reason (wlm_layout).  The multi-workgroup
# ones by enumeration of its cost model over every (words per part, row words):
# fit_ref.mc_template_pairs, asserted equal to this list in tests/test_fit_cpu.py.
_MC_G1 = ("G = 1 needs the staged words 32 * bw * wpp <= the stager threads ns <= 960, i.e. bw * wpp <= 30; "
          "C >= 2 needs ceil(wpp * nd / 2) >= 17 column chunks, i.e. wpp * nd >= 33, so nd > bw slices of the "
          "row words -- and the cost model never picks more slices than the power of two that covers bw "
          "(past it the lookups per lane stay 8 and only the chunks grow)")
UNREACHABLE = {
    "single<CPT=16,stage>": "staging needs the w tables (544 B per mask word) and the column vectors (>= 4 B "
                            "per column) in LDS: 544 * ceil(S / 32) + 4 * S >= 172,580 B for S > 8192, past "
                            "the planner's budget lds_cap = 153,600 B",
    "multi<C=2,G=1>": _MC_G1 + "; at bw * wpp <= 30 every pick has wpp * nd <= 32",
    "multi<C=4,G=1>": _MC_G1 + "; C = 4 needs wpp * nd >= 65 but nd < 2 * bw gives wpp * nd < 60",
    "multi<C=4,G=2>": "G <= 2 needs 32 * bw * wpp <= 2 * ns <= 1920, i.e. bw * wpp <= 60; C = 4 needs "
                      "ceil(wpp * nd / 2) >= 33, i.e. wpp * nd >= 65, so nd > bw: wherever a power of two "
                      "nd > bw is allowed, the cost model's pick is a smaller nd (fewer chunks per SIMD "
                      "outweigh the shorter lookups)",
}

VARIANT_CASES = fit_ref.variant_cases()


def _key(c):
    return (c.env, c.F, c.R, c.S, c.B)


@pytest.mark.parametrize("case", VARIANT_CASES, ids=_ids(VARIANT_CASES))
def test_variant_vs_oracle(case, monkeypatch):
    """One shape per reachable variant: the describe string first, then wlm_fit against the fp64
    oracle (w, losses, best epoch); for the kernels with a prologue also PreparedFit.prepare + fit,
    bitwise equal to wlm_fit."""
    desc, w, losses, best = _fit(case, monkeypatch)
    assert desc == TABLE[_key(case)]
    _compare(case, desc, w, losses, best)
    if not desc.startswith("grid"):
        pw, pl, pb = _prepared(case)
        assert torch.equal(pw, w) and torch.equal(pl, losses) and torch.equal(pb, best)


def test_variant_table_is_closed():
    """The variants pinned by TABLE and the UNREACHABLE ones are disjoint and together every name
    the dispatcher can produce (engine.WLM_VARIANTS, the library's own list)."""
    e = _eng()
    assert set(TABLE) == {_key(c) for c in VARIANT_CASES}
    pinned = {d.split()[0] for d in TABLE.values()}
    assert len(pinned) == len(TABLE)
    assert not pinned & set(UNREACHABLE)
    assert pinned | set(UNREACHABLE) == set(e.WLM_VARIANTS) == set(e.wlm_variants())


# ------------------------------------------------------------------ data and parameter corners
DATA_CASES = fit_ref.data_cases() + fit_ref.param_cases()


def _assert_dead(case, w):
    """"dead" data: a never-active column with w0 == 0 has gradient exactly 0 (sign(0) = 0, no
    decay, zero moments) and stays exactly 0.0; the always-on column stays within the bar."""
    w = w.cpu().double().numpy()
    dead, on = fit_ref.dead_columns(case.S), fit_ref.always_on_column(case.S)
    for f in range(case.F):
        assert (w[f][dead] == 0.0).all(), (case.id, w[f][dead])
        assert abs(w[f][on] - fit_ref.reference(case)[f][0][on]) <= W_ATOL


@pytest.mark.parametrize("case", DATA_CASES, ids=_ids(DATA_CASES))
def test_data_corners_vs_oracle(case, monkeypatch):
    """Row densities spread over (0.02, 0.98) with an all-on and an all-off row ("spread"), plus
    never-active columns holding w0 = 0 and an always-on column ("dead"), at (640, 300, 64)
    through every family and at (641, 1500, 64) -- the approximate KernelSHAP branch, last batch
    of one row -- through single and mc; on "dead" data also l1_lambda 0 / 1e-2 and lr 0.1."""
    desc, w, losses, best = _fit(case, monkeypatch)
    assert desc.startswith(KIND[case.env]), desc
    _compare(case, desc, w, losses, best)
    if case.data == "dead":
        _assert_dead(case, w)


@pytest.mark.parametrize("env", fit_ref.FAMILIES)
def test_negative_lr_is_bitwise_positive_lr(env, monkeypatch):
    """lr = -0.01 on "dead" data: bit for bit the fit of lr = +0.01 (the reference takes |lr|)."""
    case = fit_ref.Case(env, 1, 640, 300, 64, "dead", seed=7)
    desc, w, losses, best = _fit(case, monkeypatch)
    assert desc.startswith(KIND[env]), desc
    _, wn, ln, bn = _fit(case, monkeypatch, params={"lr": -0.01, "l1_lambda": case.lam})
    assert torch.equal(wn, w) and torch.equal(ln, losses) and torch.equal(bn, best)
    _assert_dead(case, wn)


# ------------------------------------------------------------------ rows and batch
ROW_CASES = fit_ref.row_cases()


@pytest.mark.parametrize("case", ROW_CASES, ids=_ids(ROW_CASES))
def test_rows_and_batch_vs_oracle(case, monkeypatch):
    """S = 200: fewer rows than one batch (40, 64), exactly one batch (64, 64), R = 2B + 1 (a
    last batch of one row), and B in {1, 31, 33, 63, 65} with R = 4B + 3, through every family."""
    desc, w, losses, best = _fit(case, monkeypatch)
    assert desc.startswith(KIND[case.env]), desc
    _compare(case, desc, w, losses, best)


# ------------------------------------------------------------------ columns
COLUMN_CASES = [c for c in fit_ref.column_cases() if c.env is not None]


@pytest.mark.parametrize("case", COLUMN_CASES, ids=_ids(COLUMN_CASES))
def test_column_thresholds_vs_oracle(case, monkeypatch):
    """R = 256, B = 64 at the column counts where the mask words (31 / 32 / 33), the planner
    (224 / 225: 8 words, where the multi-workgroup fit starts by default; 2048 / 2049: one grid
    chunk) and the kernels (1024 / 1025, 4096 / 4097, 8192 / 8193: columns per thread) change.
    No family is left out: the planner takes every one of these shapes under each forced family
    (under XPG_WLM=mc a shape of one mask word runs the multi-workgroup kernel with P = 1)."""
    desc, w, losses, best = _fit(case, monkeypatch)
    assert desc.startswith(KIND[case.env]), desc
    _compare(case, desc, w, losses, best)


def test_grid_threshold_vs_oracle(monkeypatch):
    """XPG_WLM unset: 16384 columns stay on the per-fit kernels, 16385 take the grid fit."""
    lo, hi = [c for c in fit_ref.column_cases() if c.env is None]
    assert (lo.S, hi.S) == (16384, 16385)
    dl, *rl = _fit(lo, monkeypatch)
    dh, *rh = _fit(hi, monkeypatch)
    assert not dl.startswith("grid") and dh.startswith("grid"), (dl, dh)
    _compare(lo, dl, *rl)
    _compare(hi, dh, *rh)


# ------------------------------------------------------------------ several fits per launch
MULTI_FIT_CASES = fit_ref.multi_fit_cases()


@pytest.mark.parametrize("case", MULTI_FIT_CASES, ids=_ids(MULTI_FIT_CASES))
def test_several_fits_per_launch_vs_oracle(case, monkeypatch):
    """8 and 9 fits in one multi-workgroup launch, every fit with its own data and compared with
    its own oracle fit; 9 fits leave workgroups of the 8-aligned grid idle."""
    desc, w, losses, best = _fit(case, monkeypatch)
    assert desc.startswith(KIND["mc"]), desc
    _compare(case, desc, w, losses, best)
