"""Inputs and references of the surrogate-fit tests (tests/test_fit_cpu.py, which needs no GPU, and
tests/test_gpu_fit_variants.py): the fp64 oracle (oracle.train_wlm), a float32 restatement of the
same algebra (train_wlm_f32: the arithmetic the reference project itself runs), the distance
between the two (e32), and every case the GPU file runs, so the CPU file asserts its conditions on
the very inputs the GPU file uses.

Bars (the project's existing ones): weights atol 1e-4, losses rtol 1e-5 against fp64.  They stand
because every case's two references agree 4x closer (e32_w <= 2.5e-5, e32_loss <= 2.5e-6): a case
whose references do not is a bad input, not a kernel finding, and its input is changed, never the
bar."""
import dataclasses
import functools
import math

import numpy as np
import torch

import oracle

W_ATOL = 1e-4      # max |w - w_fp64|
LOSS_RTOL = 1e-5   # max |loss - loss_fp64| / |loss_fp64|
E32_W = W_ATOL / 4
E32_LOSS = LOSS_RTOL / 4
MOVED = 100 * W_ATOL  # the fit must move some weight this far from w0
SPREAD = (0.02, 0.98)  # per-row keep probability of "spread" / "dead" data


@dataclasses.dataclass(frozen=True)
class Case:
    """One fit launch: F fits of R rows x S columns in batches of B under XPG_WLM=env (None:
    unset); fit f draws its data from seed + f, or from seeds[f] where `seeds` is given."""
    env: str
    F: int
    R: int
    S: int
    B: int
    data: str = "half"
    seed: int = 0
    lr: float = 0.01
    lam: float = 1e-4
    density: tuple = SPREAD
    degenerate: str = "both"  # "spread" / "dead": row 0 all-on and row 1 all-off, "off", or "none"
    seeds: tuple = ()

    @property
    def params(self):
        return {"lr": self.lr, "l1_lambda": self.lam}

    @property
    def id(self):
        s = f"{self.env or 'auto'}-F{self.F}-R{self.R}-S{self.S}-B{self.B}-{self.data}"
        if (self.lr, self.lam) != (0.01, 1e-4):
            s += f"-lr{self.lr:g}-l1{self.lam:g}"
        return s


def dead_columns(S):
    """Columns that "dead" data switches off in every row: first, middle, last."""
    return sorted({0, S // 2, S - 1})


def always_on_column(S):
    """The column "dead" data switches on in every row but the all-off one."""
    return max(1, S // 3)


def fit_inputs(R, S, B, data, seed, density=SPREAD, degenerate="both"):
    """(masks [R, S] bool, y [R] f32, kernel [R] f64 = oracle.shap_kernel(masks), w0 [S] f32).
    data "half": Bernoulli(0.5) masks.  "spread": row r keeps a column with probability p_r,
    p_r uniform in `density`; row 0 all-on and row 1 all-off (KernelSHAP weight 0) with
    degenerate = "both", only the all-off row with "off", neither with "none".  "dead": spread,
    then dead_columns(S) off in every row (row 0 is then on in every live column),
    always_on_column(S) on in every row but the all-off one, and w0 = 0.0 exactly on the dead
    columns.  B is not used to draw the data (a case's batches are cuts of one draw)."""
    rng = np.random.default_rng(seed)
    if data == "half":
        m = rng.random((R, S)) < 0.5
    elif data in ("spread", "dead"):
        m = rng.random((R, S)) < rng.uniform(density[0], density[1], (R, 1))
        if degenerate == "both":
            m[0] = True
        if degenerate in ("both", "off"):
            m[1] = False
    else:
        raise ValueError(data)
    y = rng.random(R).astype(np.float32)
    w0 = ((rng.random(S) - 0.5) * 0.05).astype(np.float32)
    if data == "dead":
        off = ~m.any(1)
        m[:, always_on_column(S)] = ~off
        m[:, dead_columns(S)] = False
        w0[dead_columns(S)] = 0.0
    for a in (m, y, w0):
        a.setflags(write=False)
    k = oracle.shap_kernel(m)
    k.setflags(write=False)
    return m, y, k, w0


def train_wlm_f32(masks, batch, outputs, kernels, w0, params):
    """oracle.train_wlm's algebra in CPU torch with every tensor float32: the batch matmul
    p = M_b w, the gradient M_b^T gp + l1 sign(w) / S + wd w, and Adam's m, v and step.  Only the
    KernelSHAP weights stay float64, as in the reference project (they lie below float32's range
    from ~130 columns on); the per-row factor gp they enter is rounded to float32 before the
    gradient matmul, as autograd rounds the gradient of a float32 prediction.  Returns
    (w f32 as f64 numpy, losses f64, first argmin epoch)."""
    m = torch.as_tensor(np.array(masks, dtype=bool))
    R, S = m.shape
    f32 = torch.float32
    y_all = torch.as_tensor(np.array(outputs, dtype=np.float32))
    k_all = torch.as_tensor(np.array(kernels, dtype=np.float64))
    w = torch.as_tensor(np.array(w0, dtype=np.float32))
    ma, va = torch.zeros(S, dtype=f32), torch.zeros(S, dtype=f32)
    lr, lam = abs(params["lr"]), params["l1_lambda"]
    b1, b2, eps, wd = 0.9, 0.999, 1e-8, 1e-2
    losses = []
    for t, r0 in enumerate(range(0, R, batch), start=1):
        mb = m[r0:r0 + batch].to(f32)
        y, kk = y_all[r0:r0 + batch], k_all[r0:r0 + batch]
        B = mb.shape[0]
        p = mb @ w
        ksum = kk.sum()
        loss = (kk[None, :] * (p[None, :] - y[:, None]).double() ** 2).mean() / ksum
        losses.append(float(loss) + float(lam * w.abs().mean()))
        gp = (2.0 * kk * (p - y.mean()).double() / (B * ksum)).to(f32)
        g = mb.T @ gp + (lam / S) * torch.sign(w) + wd * w
        ma = ma + (1 - b1) * (g - ma)
        va = b2 * va + (1 - b2) * g * g
        w = w - (lr / (1 - b1 ** t)) * ma / (va.sqrt() / math.sqrt(1 - b2 ** t) + eps)
        assert w.dtype == f32 and ma.dtype == f32 and va.dtype == f32 and p.dtype == f32
    losses = np.asarray(losses)
    return w.double().numpy(), losses, int(np.argmin(losses))


@functools.lru_cache(maxsize=None)
def inputs(case):
    """fit_inputs of each of the case's F fits."""
    return tuple(fit_inputs(case.R, case.S, case.B, case.data, case.seeds[f] if case.seeds else case.seed + f,
                            case.density, case.degenerate) for f in range(case.F))


@functools.lru_cache(maxsize=None)
def reference(case):
    """Per fit (w fp64, losses, best epoch) of oracle.train_wlm, computed once per case."""
    out = []
    for m, y, k, w0 in inputs(case):
        w, l, b = oracle.train_wlm(m, case.B, y, k, w0, case.params)
        w.setflags(write=False)
        l.setflags(write=False)
        out.append((w, l, b))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference_f32(case):
    return tuple(train_wlm_f32(m, case.B, y, k, w0, case.params) for m, y, k, w0 in inputs(case))


def e32(case):
    """(max |w_f32 - w_fp64|, max relative |loss_f32 - loss_fp64|) over the case's fits."""
    ew = el = 0.0
    for (w, l, _), (w32, l32, _) in zip(reference(case), reference_f32(case)):
        ew = max(ew, float(np.abs(w32 - w).max()))
        el = max(el, float(np.max(np.abs(l32 - l) / np.abs(l))))
    return ew, el


def best_epochs(losses):
    """(rule, allowed epochs) for a fit's best epoch given the fp64 losses: "strict" -- the two
    smallest differ by more than the loss bar, so the kernel's first argmin must be the oracle's;
    "margin" -- they do not, and any epoch whose loss is within the bar of the smallest passes."""
    l = np.asarray(losses)
    lo = float(l.min())
    tol = LOSS_RTOL * abs(lo)
    near = [int(i) for i in np.nonzero(l <= lo + tol)[0]]
    if len(near) == 1:
        return "strict", [int(np.argmin(l))]
    return "margin", near


# ------------------------------------------------------------------ the cases of the GPU file
NARROW = dict(data="spread", density=(0.3, 0.7), degenerate="none")

# One shape per fit variant (engine.WLM_VARIANTS): small shapes that reach each name, from a scan
# of engine.wlm_describe over (cols, batch, n_fits, XPG_WLM) on the MI355X;
# tests/test_gpu_fit_variants.py holds the describe string each must report.  "half" data, 3-5
# steps; the seed (and the step count) is the first of a search from 100 up whose references meet
# the conditions of tests/test_fit_cpu.py with the fit moved >= 0.012 (at lr = 0.01 a fit over
# thousands of Bernoulli(0.5) columns mostly swings every weight by +-lr together).
VARIANT_SHAPES = [  # (XPG_WLM, F, S, B, steps, seed)
    ("single", 1, 100, 32, 4, 100),    # k_wlm_fit<1, stage>
    ("single", 1, 1025, 32, 4, 103),   # <2, stage>: > 1024 columns
    ("single", 1, 2049, 32, 4, 103),   # <4, stage>
    ("single", 1, 4097, 32, 4, 101),   # <8, stage>
    ("single", 1, 1000, 352, 5, 105),  # <1, nostage>: cols x row words > the staging buffer
    ("single", 1, 1500, 256, 4, 101),  # <2, nostage>
    ("single", 1, 4096, 33, 4, 102),   # <4, nostage>
    ("single", 1, 6144, 32, 4, 110),   # <8, nostage>: the staged image is past the LDS budget
    ("single", 1, 8193, 32, 4, 103),   # <16, nostage>
    ("mc", 1, 100, 32, 4, 100),        # k_wlm_fit_mc<1, 1>
    ("mc", 1, 128, 352, 4, 100),       # <1, 2>: 2 words per part x 11 row words
    ("mc", 1, 200, 400, 4, 100),       # <1, 4>: 3 x 13
    (None, 1, 4608, 160, 4, 105),      # <2, 2>: 9 x 5, 4 column-row slices
    (None, 1, 2560, 288, 3, 105),      # <2, 4>: 5 x 9, 8 slices
    (None, 33, 12450, 32, 3, 100),     # <4, 4>: 65 words per part (33 fits leave 6 parts per fit)
    ("grid3", 1, 100, 32, 4, 100),
    ("grid", 1, 100, 32, 4, 100),
]


# the 33 seeds from 100 up whose one fit at (96, 12450, 32) meets the conditions on its own
SEEDS_33 = (100, 101, 102, 104, 105, 106, 108, 109, 110, 112, 113, 114, 115, 117, 118, 119, 120, 121, 122, 124, 126,
            127, 129, 130, 131, 132, 133, 134, 135, 136, 137, 138, 139)


def variant_case(env, F, S, B, steps, seed):
    """"half" data, but the 33-fit case: among 33 x 12,450 Bernoulli(0.5) columns some column's
    gradient is noise-signed in every draw tried (e32_w ~ 3e-3, Adam normalising it), so it takes
    the narrow density range, and each of its fits a seed that passes alone (about one draw in
    four does not: a loss 1e-5 apart between float32 and fp64)."""
    if F > 1:
        assert F == len(SEEDS_33)
        return Case(env, F, steps * B, S, B, seed=seed, seeds=SEEDS_33, **NARROW)
    return Case(env, F, steps * B, S, B, "half", seed=seed)


def variant_cases():
    return [variant_case(*v) for v in VARIANT_SHAPES]


def mc_template_pairs():
    """Every (C, G) of k_wlm_fit_mc<C, G> the planner's cost model (wlm_layout in csrc/xpgnn.hip)
    can pick, by enumeration over words per part (1..256) and row words (1..32): C = column chunks
    per lane (3 -> 4) under the cheapest slice count nd, G = staged words per stager (1 / 2 / 4).
    The pick depends on (wpp, bw) only: staged words = 32 bw wpp whatever the batch within its row
    word."""
    cdiv = lambda a, b: -(-a // b)  # noqa: E731
    pairs = set()
    for bw in range(1, 33):
        nrb = cdiv(bw, 2)
        ns = 1024 - 64 * nrb if nrb <= 8 else 1024
        for wpp in range(1, 257):
            best = None
            for lg, nd in enumerate((1, 2, 4, 8, 16)):
                chunks = cdiv(wpp * 32, 64 // nd)
                cpl = cdiv(chunks, 16)
                if cpl > 4:
                    continue
                look = cdiv(bw, nd) * 8
                cost = cdiv(chunks, 4) * (look * 4 + 100 + 10 * lg) + cdiv(look, 16) * 400
                if best is None or cost < best[0]:
                    best = (cost, 4 if cpl == 3 else cpl)
            stage = 32 * bw * wpp
            if best is None or stage > 4 * ns:
                continue
            pairs.add((best[1], 1 if stage <= ns else 2 if stage <= 2 * ns else 4))
    return pairs


FAMILIES = ("single", "mc", "grid3", "grid")
KIND = {"single": "single<", "mc": "multi<", "grid3": "grid3 ", "grid": "grid_fused "}


def data_cases():
    """"spread" and "dead" data at (640, 300, 64) through every family, and at (641, 1500, 64)
    (the approximate KernelSHAP branch, M > 1000; a last batch of one row) through single and mc.
    At 1,500 columns "spread" carries the all-off row only: the approximate branch gives an all-on
    row the weight M / (c k (M - k)) with M - k = -1, a negative number that outweighs its whole
    batch, and sum(kernel) > 0 is a condition of every case ("dead" has no all-on row)."""
    out = [Case(env, 1, 640, 300, 64, data, seed=7) for env in FAMILIES for data in ("spread", "dead")]
    out += [Case(env, 1, 641, 1500, 64, data, seed=8, degenerate="off")
            for env in ("single", "mc") for data in ("spread", "dead")]
    return out


def param_cases():
    """l1_lambda 0 and 1e-2, lr 0.1 on "dead" data; lr = -0.01 is compared with +0.01 bit for bit
    (tests/test_gpu_fit_variants.py runs it beside the plain "dead" case of data_cases)."""
    out = []
    for env in FAMILIES:
        out += [Case(env, 1, 640, 300, 64, "dead", seed=7, lam=0.0),
                Case(env, 1, 640, 300, 64, "dead", seed=7, lam=1e-2),
                Case(env, 1, 640, 300, 64, "dead", seed=7, lr=0.1)]
    return out


def row_cases():
    """R < B, R == B, R = 2B + 1 and B in {1, 31, 33, 63, 65} with R = 4B + 3, S = 200.  B = 1:
    no all-on / all-off row (a batch needs sum(kernel) > 0).  lr = 0.02: a fit of one step moves
    every weight by lr |g| / (|g| + eps) < lr, which at lr = 0.01 is just short of the 0.01 the
    fit must move."""
    shapes = [(40, 64), (64, 64), (129, 64)] + [(4 * b + 3, b) for b in (1, 31, 33, 63, 65)]
    return [Case(env, 1, R, 200, B, "spread", seed=9, lr=0.02, degenerate="both" if B > 1 else "none")
            for env in FAMILIES for R, B in shapes]


def column_cases():
    """R = 256, B = 64 at the word, planner and kernel thresholds of the column count, on the
    narrow density range (0.3, 0.7): four steps over Bernoulli(0.5) columns move no weight 0.01
    at several of these sizes, and at 16,384 columns their KernelSHAP weights underflow to 0."""
    out = [Case(env, 1, 256, S, 64, seed=10, **NARROW)
           for env in ("single", "mc") for S in (2, 3, 31, 32, 33, 224, 225, 1024, 1025, 4096, 4097)]
    out += [Case(env, 1, 256, S, 64, seed=10, **NARROW) for env in ("grid3", "grid") for S in (2048, 2049, 8192, 8193)]
    out += [Case(None, 1, 256, S, 64, seed=10, **NARROW) for S in (16384, 16385)]
    return out


def multi_fit_cases():
    """8 and 9 fits in one multi-workgroup launch, each fit with its own data."""
    return [Case("mc", F, 640, 300, 64, "spread", seed=20) for F in (8, 9)]


def all_cases():
    seen, out = set(), []
    for c in variant_cases() + data_cases() + param_cases() + row_cases() + column_cases() + multi_fit_cases():
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out
