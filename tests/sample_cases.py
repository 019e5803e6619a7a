"""The seeded cases of the sampling tests and the fp64 statement of the rule `setok_sample_rows` implements (include/setok_hip.h, "Sampling"):
temperature, then top-k (ties at the threshold kept), then top-p (keep a token iff the mass of the kept tokens with a STRICTLY larger score is
< top_p), probabilities by softmax over the kept set, the draw by inverse CDF in index order.

The cases are built so that the reference alone decides every outcome:
  top_k  comes from a fixed list;
  top_p  is, per row, the fp32 midpoint of a gap wider than 1e-3 between consecutive "mass above" values of that row, below a score that no
         other token of the row shares (a call has ONE top_p, so a
         top-p case is run row by row; that a row alone equals the row in a batch is an exact property the GPU tests check separately);
  u      is, per row, the fp32 midpoint of the CDF interval of a token whose probability exceeds 1e-3.
tests/golden/make_golden_sample.py runs HuggingFace's own logits warpers on the same cases and asserts that this rule gives HF's kept set.
Logits are regenerated from seeds (torch's CPU generator), never stored."""
from __future__ import annotations

import functools

import numpy as np
import torch

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
PAD = 8                                             # the GPU tests run at ld = V + PAD with NaN in the pad columns
MIN_GAP = 1e-3                                      # top_p sits in the middle of a gap wider than this; u at least MIN_GAP / 2 inside its interval
MIN_P = 1e-3


def _c(V, rows, dt, T, k=0, p=False, ninf=False):
    return dict(V=V, rows=rows, dt=dt, T=T, k=k, p=p, ninf=ninf)


# V in {1, 7, 257, 32000, 128256} x rows in {1, 3, 33} x three element types x T in {0.1, 1, 2} x filters {none, top-k 1 / 2 / 50 / V + 5, top-p, both}.
# The GPU tests hold the probability error of a case to twice HuggingFace's own fp32-against-fp64 error ON THAT CASE, a maximum over the case's
# non-zero entries.  Over two or three entries that maximum is the luck of a few fp32 roundings (one rounding of p = 0.5 errs by anything in
# [0, 3e-8]), so a case whose filter leaves only a few tokens per row has 33 rows; the cases of 1 and 3 rows are those that keep hundreds of
# entries per row, or a single one (p = 1 exactly, for HF and for the kernel alike).
CASES = {
    "v1_r1_fp32_T1": _c(1, 1, "fp32", 1.0),
    "v1_r3_bf16_T0.1_k1": _c(1, 3, "bf16", 0.1, k=1),
    "v1_r1_fp16_T2_p": _c(1, 1, "fp16", 2.0, p=True),
    "v7_r33_fp16_T2": _c(7, 33, "fp16", 2.0),
    "v7_r33_fp32_T1_k2": _c(7, 33, "fp32", 1.0, k=2),
    "v7_r1_bf16_T1_p": _c(7, 1, "bf16", 1.0, p=True),
    "v257_r3_bf16_T1": _c(257, 3, "bf16", 1.0),
    "v257_r33_fp32_T0.1_k50": _c(257, 33, "fp32", 0.1, k=50),
    "v257_r33_fp16_T2_p": _c(257, 33, "fp16", 2.0, p=True, ninf=True),
    "v257_r33_fp32_T1_k50_p": _c(257, 33, "fp32", 1.0, k=50, p=True),
    "v257_r1_fp32_T1_k262": _c(257, 1, "fp32", 1.0, k=262),
    "v32000_r33_bf16_T1": _c(32000, 33, "bf16", 1.0),
    "v32000_r3_fp32_T0.1": _c(32000, 3, "fp32", 0.1),
    "v32000_r33_fp16_T2_k50": _c(32000, 33, "fp16", 2.0, k=50),
    "v32000_r33_bf16_T1_p": _c(32000, 33, "bf16", 1.0, p=True, ninf=True),
    "v32000_r33_fp32_T2_k50_p": _c(32000, 33, "fp32", 2.0, k=50, p=True),
    "v32000_r1_bf16_T0.1_k1": _c(32000, 1, "bf16", 0.1, k=1),
    "v32000_r33_bf16_T1_k2": _c(32000, 33, "bf16", 1.0, k=2),
    "v32000_r1_fp32_T1_k32005": _c(32000, 1, "fp32", 1.0, k=32005),
    "v128256_r3_bf16_T1": _c(128256, 3, "bf16", 1.0, ninf=True),
    "v128256_r33_fp32_T2_k50": _c(128256, 33, "fp32", 2.0, k=50),
    "v128256_r33_fp16_T0.1_p": _c(128256, 33, "fp16", 0.1, p=True),
    "v128256_r33_bf16_T1_k50_p": _c(128256, 33, "bf16", 1.0, k=50, p=True, ninf=True),
    "v128256_r1_fp32_T1_k128261": _c(128256, 1, "fp32", 1.0, k=128261),
}
SEEDS = {name: 4000 + i for i, name in enumerate(CASES)}


def filtered(case) -> bool:
    """Whether the case's kept set is a proper filter (top-k below V, or top-p): the fixture stores the kept set itself then."""
    return case["p"] or 0 < case["k"] < case["V"]


def logits(name) -> torch.Tensor:
    """(rows, V) in the case's element type: N(0, 3^2) rounded to the type (many ties in 16 bits), a tenth of the entries -inf where `ninf`."""
    c = CASES[name]
    g = torch.Generator().manual_seed(SEEDS[name])
    x = torch.randn(c["rows"], c["V"], generator=g) * 3.0
    if c["ninf"]:
        dead = torch.rand(c["rows"], c["V"], generator=g) < 0.1
        dead[:, c["V"] // 2] = False                                   # every row keeps a finite entry
        x = x.masked_fill(dead, float("-inf"))
    return x.to(DTYPES[c["dt"]])


# ---- the rule in fp64 (numpy), one row at a time ---------------------------------------------------------------------------------------------
def scores(x_row: torch.Tensor, T: float) -> np.ndarray:
    return x_row.double().numpy() / float(T)


def topk_keep(s: np.ndarray, top_k: int) -> np.ndarray:
    V = s.size
    if 0 < top_k < V:
        return s >= np.partition(s, V - top_k)[V - top_k]
    return np.ones(V, bool)


def softmax_over(s: np.ndarray, keep: np.ndarray) -> np.ndarray:
    e = np.where(keep, np.exp(s - s[keep].max()), 0.0)
    return e / e.sum()


def mass_above(s: np.ndarray, keep: np.ndarray) -> np.ndarray:
    """Per token: the probability (over `keep`) of the kept tokens with a strictly larger score."""
    V = s.size
    p = softmax_over(s, keep)
    order = np.argsort(-s, kind="stable")
    ps, ss = p[order], s[order]
    before = np.cumsum(ps) - ps
    first = np.r_[True, ss[1:] != ss[:-1]]
    start = np.maximum.accumulate(np.where(first, np.arange(V), 0))    # the first position of every run of equal scores
    out = np.empty(V)
    out[order] = before[start]
    return out


def keep_rule(s: np.ndarray, top_k: int, top_p: float) -> np.ndarray:
    keep = topk_keep(s, top_k)
    if top_p < 1.0:
        keep = keep & (mass_above(s, keep) < top_p)
    return keep


def intervals(p: np.ndarray):
    """The CDF interval [lo, hi) of every token, in index order."""
    hi = np.cumsum(p)
    return hi - p, hi


def draw(p: np.ndarray, u: float) -> int:
    lo, hi = intervals(p)
    return int(np.searchsorted(hi, u, side="right"))


def choose_top_p(s: np.ndarray, top_k: int, rng) -> np.float32:
    keep = topk_keep(s, top_k)
    vals, count = np.unique(np.r_[mass_above(s, keep)[keep], 1.0], return_counts=True)
    # twice the stated minimum: the fp32 rounding of the midpoint changes nothing.  The last kept score must be no run of equal scores: HF cuts
    # inside such a run by sort position, the rule here keeps the run together, and only without one do both name the same set.
    gaps = np.nonzero((np.diff(vals) > 2 * MIN_GAP) & (count[:-1] == 1))[0]
    assert gaps.size, "no gap for top_p"
    j = int(gaps[rng.integers(gaps.size)])
    return np.float32(0.5 * (vals[j] + vals[j + 1]))


def choose_u(p: np.ndarray, rng):
    lo, hi = intervals(p)
    cand = np.nonzero(p > 2 * MIN_P)[0]
    assert cand.size, "no token above the probability floor"
    t = int(cand[rng.integers(cand.size)])
    return np.float32(0.5 * (lo[t] + hi[t])), t


@functools.lru_cache(maxsize=None)
def build(name):
    """Per row of the case: top_p (1.0 = off), u, the expected token, the kept mask and the fp64 probabilities — from the rule above alone."""
    c = CASES[name]
    x = logits(name)
    rows = []
    for r in range(c["rows"]):
        rng = np.random.default_rng(SEEDS[name] * 100 + r)
        s = scores(x[r], c["T"])
        top_p = choose_top_p(s, c["k"], rng) if c["p"] else np.float32(1.0)
        keep = keep_rule(s, c["k"], float(top_p))
        p = softmax_over(s, keep)
        u, tok = choose_u(p, rng)
        rows.append(dict(top_p=top_p, u=u, token=tok, keep=keep, p=p))
    return rows


# ---- the fixed-point model of the kernel's arithmetic on the CPU (numpy's fp32 exp in place of the device's) ------------------------------------
def fixed_point_draw(x_row: torch.Tensor, T: float, top_k: int, top_p: float, u: float):
    """(token, probs) as setok_sample_rows defines them: fp32 scores, integer weights rint(exp(s - max) * 2^32), integer sums."""
    s = (x_row.float().numpy() / np.float32(T)).astype(np.float32)
    V = s.size
    m = s.max()
    w_all = np.rint(np.exp((s - m).astype(np.float32)).astype(np.float32).astype(np.float64) * 2.0 ** 32).astype(np.uint64)
    keep = topk_keep(s.astype(np.float64), top_k)
    if top_p < 1.0:
        w = np.where(keep, w_all, 0).astype(np.uint64)
        order = np.argsort(-s, kind="stable")
        ws, ss = w[order], s[order]
        before = np.cumsum(ws) - ws
        first = np.r_[True, ss[1:] != ss[:-1]]
        start = np.maximum.accumulate(np.where(first, np.arange(V), 0))
        above = np.empty(V, np.uint64)
        above[order] = before[start]
        keep = keep & (above.astype(np.float64) < float(np.float32(top_p)) * float(w.sum()))
    w = np.where(keep, w_all, 0).astype(np.uint64)
    W = int(w.sum())
    u24 = int(np.float32(min(max(float(u), 0.0), 1.0 - 2.0 ** -24)) * np.float32(2.0 ** 24))
    target = (W * u24) >> 24
    hi = np.cumsum(w)
    return int(np.searchsorted(hi, np.uint64(target), side="right")), w.astype(np.float64) / W
