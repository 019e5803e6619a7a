"""Golden vectors for sampled token selection (tests/golden/sample.npz).

Run where `transformers` is available:  python tests/golden/make_golden_sample.py

For every case of tests/sample_cases.py (logits regenerated from seeds, not stored) HuggingFace's own TemperatureLogitsWarper, TopKLogitsWarper
and TopPLogitsWarper run in that order, once in fp64 and once in fp32 (HF's generation loop casts the step's logits to fp32 before its
processors), followed by softmax.  Stored per case:
    top_p (rows,) f32 (1.0 = off)   u (rows,) f32   tokens (rows,) i64: the token HF's fp64 distribution draws with u by inverse CDF in index order
    kept_count (rows,)              hf_err (2,): max-norm and rms of HF's fp32 probabilities against its fp64 ones — the yardstick of the GPU tests
    filtered cases:   kept_row / kept_idx (the kept set, flattened) and kept_p (their fp64 probabilities)
    unfiltered cases: top_idx / top_p64 (rows, 8): the eight most probable tokens and their fp64 probabilities (the full distribution of a
                      (33, 128256) case does not fit a committed file; the GPU tests recompute it with sample_cases' fp64 rule, which is asserted
                      here to agree with HF's to 1e-12 on every case)
Asserted here, per row: sample_cases' rule gives HF's kept set, in fp64 and in fp32 alike; its probabilities agree with HF's fp64 ones to 1e-12;
u lies at least 5e-4 inside the CDF interval of its token; the fixed-point CPU model of the kernel draws HF's token."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import golden_io                                   # noqa: E402
import sample_cases as S                           # noqa: E402

TOP = 8


def hf_probs(x, T, top_k, top_p, dtype):
    """x (1, V) -> (HF's kept mask, HF's warped distribution) computed in `dtype`, as numpy (V,)."""
    scores = x.to(dtype)
    if T != 1.0:
        scores = TemperatureLogitsWarper(float(T))(None, scores)
    if top_k > 0:
        scores = TopKLogitsWarper(top_k=int(top_k))(None, scores)
    if top_p < 1.0:
        scores = TopPLogitsWarper(top_p=float(top_p))(None, scores)
    return (scores[0] > float("-inf")).numpy(), torch.softmax(scores, dim=-1)[0].double().numpy()


def main():
    out, model_hits, draws = {}, 0, 0
    worst32 = 0.0
    for name, c in S.CASES.items():
        x = S.logits(name)
        rows = S.build(name)
        err_max, err_sq, tokens = 0.0, 0.0, []
        kept_row, kept_idx, kept_p, top_idx, top_p64 = [], [], [], [], []
        for r, row in enumerate(rows):
            keep64, p64 = hf_probs(x[r:r + 1], c["T"], c["k"], float(row["top_p"]), torch.float64)
            keep32, p32 = hf_probs(x[r:r + 1], c["T"], c["k"], float(row["top_p"]), torch.float32)
            finite = np.isfinite(S.scores(x[r], c["T"]))             # (an -inf logit is "kept" by a rule without a filter and has probability 0)
            assert np.array_equal(row["keep"] & finite, keep64), (name, r, "kept set fp64")
            assert np.array_equal(keep32, keep64), (name, r, "kept set fp32")
            assert np.abs(row["p"] - p64).max() < 1e-12, (name, r, np.abs(row["p"] - p64).max())
            lo, hi = S.intervals(p64)
            tok = S.draw(p64, float(row["u"]))
            assert tok == row["token"] and lo[tok] + 5e-4 <= float(row["u"]) <= hi[tok] - 5e-4, (name, r)
            mt, mp = S.fixed_point_draw(x[r], c["T"], c["k"], float(row["top_p"]), float(row["u"]))
            model_hits += int(mt == tok)
            draws += 1
            worst32 = max(worst32, float(np.abs(mp - p64).max()))
            e = p32 - p64
            err_max, err_sq = max(err_max, float(np.abs(e).max())), err_sq + float((e * e).sum())
            tokens.append(tok)
            if S.filtered(c):
                idx = np.nonzero(row["keep"])[0]
                kept_row.append(np.full(idx.size, r, np.int32)); kept_idx.append(idx.astype(np.int32)); kept_p.append(p64[idx])
            else:
                best = np.argsort(-p64, kind="stable")[:TOP]
                best = np.r_[best, np.full(TOP - best.size, -1)]
                top_idx.append(best.astype(np.int32)); top_p64.append(np.where(best >= 0, p64[np.maximum(best, 0)], 0.0))
        out[name + ":top_p"] = np.array([row["top_p"] for row in rows], np.float32)
        out[name + ":u"] = np.array([row["u"] for row in rows], np.float32)
        out[name + ":tokens"] = np.array(tokens, np.int64)
        out[name + ":kept_count"] = np.array([int(row["keep"].sum()) for row in rows], np.int64)
        out[name + ":hf_err"] = np.array([err_max, (err_sq / (c["rows"] * c["V"])) ** 0.5], np.float64)
        if S.filtered(c):
            out[name + ":kept_row"], out[name + ":kept_idx"] = np.concatenate(kept_row), np.concatenate(kept_idx)
            out[name + ":kept_p"] = np.concatenate(kept_p)
        else:
            out[name + ":top_idx"], out[name + ":top_p64"] = np.stack(top_idx), np.stack(top_p64)
        print(f"{name}: HF fp32 vs fp64 max {err_max:.3e} rms {out[name + ':hf_err'][1]:.3e}  kept {out[name + ':kept_count'].tolist()[:3]}")
    print(f"fixed-point CPU model: {model_hits} of {draws} draws equal HF's; worst probability error {worst32:.3e}")
    assert model_hits == draws
    files = golden_io.save(os.path.join(HERE, "sample.npz"), **out)
    print([(os.path.basename(f), os.path.getsize(f)) for f in files])


if __name__ == "__main__":
    main()
