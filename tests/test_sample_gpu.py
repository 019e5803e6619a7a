"""Sampled token selection on a real MI355X: setok_sample_rows against HuggingFace's logits warpers (tests/golden/sample.npz,
tests/golden/make_golden_sample.py; the cases and the fp64 rule are tests/sample_cases.py), its exact properties, and
`SetokimLlamaPrefill.generate(sampler=...)` on the small cases of tests/llama_bwd_cases.py.  `pytest -m gpu`.

Probability error.  The bound is 2 x HF's own fp32-against-fp64 error on the case + 2^-32, in max-norm and in rms (the kernel rounds the scaled
score once and the exponential once, as HF's fp32 path does, with another exp, hence the factor; 2^-32 is the weight grid).  The measured values
are logged through SETOK_PARITY_LOG (profiles/sample_parity.txt)."""
import os

import numpy as np
import pytest
import torch

import golden_io
import llama_bwd_cases as C
import sample_cases as S
import setok_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from setok_amd import ops
    from setok_amd.generation import Sampler
    from setok_amd.llama import SetokimLlamaPrefill

DEV = "cuda"
GRID = 2.0 ** -32
U_MAX = 1.0 - 2.0 ** -24


def _log(label, *nums):
    path = os.environ.get("SETOK_PARITY_LOG")
    if path:
        test = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]
        with open(path, "a") as f:
            f.write(f"{test}\t{label}\t" + "\t".join(f"{n:.3e}" for n in nums) + "\n")
    print(label, *[f"{n:.3e}" for n in nums])


def _wide(x):
    """x (rows, V) on the device as a view of a (rows, V + PAD) buffer whose pad columns hold NaN: a kernel that reads past V returns -1."""
    rows, V = x.shape
    w = torch.full((rows, V + S.PAD), float("nan"), dtype=x.dtype)
    w[:, :V] = x
    return w.to(DEV)[:, :V]


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return golden_io.load(os.path.join(golden_dir, "sample.npz"))


# ---- parity against the fixture ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.CASES))
def test_tokens_support_and_probabilities_against_hf(golden, name):
    c, z = S.CASES[name], golden
    rows, V = c["rows"], c["V"]
    built = S.build(name)                                              # the fp64 rule; tests/test_sample_cpu.py holds it to the fixture
    xd = _wide(S.logits(name))
    u, top_p = torch.from_numpy(z[name + ":u"]).to(DEV), z[name + ":top_p"]
    probs = torch.full((rows, V), -1.0, dtype=torch.float32, device=DEV)
    if c["p"]:                                                         # one top_p per call: row by row
        tok = torch.cat([ops.sample_rows(xd[r:r + 1], u[r:r + 1], c["T"], c["k"], float(top_p[r]), probs=probs[r:r + 1]) for r in range(rows)])
    else:
        tok = ops.sample_rows(xd, u, c["T"], c["k"], 1.0, probs=probs)
    assert tok.dtype == torch.int64 and tok.shape == (rows,)
    got = probs.double().cpu().numpy()
    assert np.array_equal(tok.cpu().numpy(), z[name + ":tokens"]), (tok.cpu().tolist(), z[name + ":tokens"].tolist())
    p64 = np.stack([b["p"] for b in built])
    keep = np.stack([b["keep"] for b in built])
    if S.filtered(c):                                                  # HF's own kept set
        keep = np.zeros_like(keep)
        keep[z[name + ":kept_row"], z[name + ":kept_idx"]] = True
    assert (got >= 0).all() and not (got[~keep] > 0).any()             # the support is a subset of HF's ...
    missing = keep & (got == 0)
    assert not missing.any() or p64[missing].max() < GRID              # ... and what is missing from it lies below the weight grid
    assert np.abs(got.sum(1) - 1.0).max() < 1e-5
    e = got - p64
    err_max, err_rms = float(np.abs(e).max()), float(np.sqrt((e * e).mean()))
    hf_max, hf_rms = (float(v) for v in z[name + ":hf_err"])
    _log(f"{name}: max err, bound, rms err, bound", err_max, 2 * hf_max + GRID, err_rms, 2 * hf_rms + GRID)
    assert err_max <= 2 * hf_max + GRID and err_rms <= 2 * hf_rms + GRID, (err_max, hf_max, err_rms, hf_rms)


# ---- exact properties ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,V", [(33, 32000), (3, 128256), (5, 257)])
def test_top_k_1_and_a_tiny_top_p_are_the_argmax_for_any_u(rows, V):
    x = _rand(rows, V, seed=21) * 3.0
    top2 = x.topk(2, dim=1).values
    assert (top2[:, 0] > top2[:, 1]).all()                             # fp32 random rows: no tie at the maximum
    xd = _wide(x)
    want = ops.argmax_rows(xd)
    for seed, T in ((1, 1.0), (2, 0.1), (3, 2.0)):
        u = torch.rand(rows, generator=torch.Generator().manual_seed(seed)).to(DEV)
        assert torch.equal(ops.sample_rows(xd, u, T, 1, 1.0), want)
        assert torch.equal(ops.sample_rows(xd, u, T, 0, 1e-6), want)
        assert torch.equal(ops.sample_rows(xd, u, T, 1, 1e-6), want)
    for edge in (0.0, U_MAX, 1.0, -1.0, 2.0):                          # u outside [0, 1) is clamped
        assert torch.equal(ops.sample_rows(xd, torch.full((rows,), edge, device=DEV), 1.0, 1, 1.0), want)


@pytest.mark.parametrize("dt", list(S.DTYPES))
@pytest.mark.parametrize("V,k", [(7, 0), (257, 50), (32000, 50), (128256, 50)])
def test_u_0_draws_the_first_kept_index_and_the_largest_u_the_last(dt, V, k):
    rows = 3
    x = (_rand(rows, V, seed=31 + V) * 2.0).to(S.DTYPES[dt])
    xd = _wide(x)
    first, last = [], []
    for r in range(rows):
        s = S.scores(x[r], 1.0)
        keep = S.keep_rule(s, k, 1.0)
        assert (s[keep].max() - s[keep].min()) < 20.0                  # every kept weight is far above the 2^-33 floor
        idx = np.nonzero(keep)[0]
        first.append(int(idx[0])); last.append(int(idx[-1]))
    assert ops.sample_rows(xd, torch.zeros(rows, device=DEV), 1.0, k, 1.0).tolist() == first
    assert ops.sample_rows(xd, torch.full((rows,), U_MAX, device=DEV), 1.0, k, 1.0).tolist() == last
    assert ops.sample_rows(xd, torch.full((rows,), 1.0, device=DEV), 1.0, k, 1.0).tolist() == last


@pytest.mark.parametrize("V,T,k,top_p", [(4099, 2.0, 0, 1.0), (4099, 1.0, 50, 0.9), (257, 1.0, 0, 1.0)])
def test_a_grid_of_sorted_u_draws_in_index_order_and_fills_every_interval(V, T, k, top_p):
    """One row, 4096 sorted u = (j + 0.5) / 4096.  The inverse CDF runs in index order, so the drawn indices are non-decreasing (a wrong scan breaks
    that); and a token is drawn as often as grid points lie in its fp64 interval, within one grid point per interval end (the kernel's CDF differs
    from the fp64 one by the probability error, ~1e-6, far less than the grid's 2.4e-4)."""
    n = 4096
    x = _rand(1, V, seed=41) * 3.0
    s = S.scores(x[0], T)
    keep = S.keep_rule(s, k, top_p)
    if top_p < 1.0:                                                    # the shared top_p must decide the kept set on its own
        assert np.abs(S.mass_above(s, S.topk_keep(s, k)) - top_p).min() > 1e-4
    p = S.softmax_over(s, keep)
    lo, hi = S.intervals(p)
    grid = (np.arange(n) + 0.5) / n
    want = np.searchsorted(grid, hi, side="left") - np.searchsorted(grid, lo, side="left")       # grid points in [lo, hi)
    xd = _wide(x.repeat(n, 1))
    tok = ops.sample_rows(xd, torch.from_numpy(grid.astype(np.float32)).to(DEV), T, k, top_p).cpu().numpy()
    assert tok.min() >= 0 and keep[tok].all()
    assert (np.diff(tok) >= 0).all()
    count = np.bincount(tok, minlength=V)
    assert np.abs(count - want).max() <= 2, int(np.abs(count - want).max())
    assert len(np.unique(tok)) >= 8                                    # (the row is no one-token distribution)


@pytest.mark.parametrize("dt", list(S.DTYPES))
@pytest.mark.parametrize("V", [32000, 128256])
def test_repeated_calls_agree_and_a_row_alone_equals_the_row_in_the_batch(dt, V):
    rows = 33 if V == 32000 else 5
    xd = _wide((_rand(rows, V, seed=51) * 3.0).to(S.DTYPES[dt]))
    u = torch.rand(rows, generator=torch.Generator().manual_seed(52)).to(DEV)
    for T, k, top_p in ((0.8, 50, 0.9), (1.0, 0, 1.0), (1.0, 0, 0.7)):
        runs = []
        for _ in range(3):
            probs = torch.empty(rows, V, dtype=torch.float32, device=DEV)
            runs.append((ops.sample_rows(xd, u, T, k, top_p, probs=probs), probs))
        for tok, probs in runs[1:]:
            assert torch.equal(tok, runs[0][0]) and torch.equal(probs, runs[0][1])
        assert int(runs[0][0].min()) >= 0
        for r in (0, rows // 2, rows - 1):
            probs = torch.empty(1, V, dtype=torch.float32, device=DEV)
            alone = ops.sample_rows(xd[r:r + 1], u[r:r + 1], T, k, top_p, probs=probs)
            assert int(alone[0]) == int(runs[0][0][r]) and torch.equal(probs[0], runs[0][1][r])
        assert torch.equal(ops.sample_rows(xd, u, T, k, top_p), runs[0][0])                     # without probs: the same tokens


@pytest.mark.parametrize("V", [257, 32000, 128256])
def test_an_inf_entry_is_never_drawn(V):
    n = 512
    x = _rand(1, V, seed=61)
    dead = torch.rand(1, V, generator=torch.Generator().manual_seed(62)) < 0.9
    dead[0, V // 3] = False
    x = x.masked_fill(dead, float("-inf")).to(torch.bfloat16)
    u = torch.rand(n, generator=torch.Generator().manual_seed(63)).to(DEV)
    u[0], u[1] = 0.0, U_MAX
    xd = _wide(x.repeat(n, 1))
    for T, k, top_p in ((1.0, 0, 1.0), (2.0, V - 1, 1.0), (1.0, 0, 0.99)):
        probs = torch.empty(n, V, dtype=torch.float32, device=DEV) if V <= 32000 else None
        tok = ops.sample_rows(xd, u, T, k, top_p, probs=probs).cpu()
        assert int(tok.min()) >= 0 and not dead[0, tok].any()
        assert len(tok.unique()) >= 8
        if probs is not None:
            assert float(probs[:, dead[0].to(DEV)].max()) == 0.0


@pytest.mark.parametrize("dt", list(S.DTYPES))
@pytest.mark.parametrize("V", [7, 32000, 128256])
def test_bad_rows_give_minus_one_and_leave_their_neighbours_alone(dt, V):
    rows = 7
    x = (_rand(rows, V, seed=71) * 3.0).to(S.DTYPES[dt])
    u = torch.rand(rows, generator=torch.Generator().manual_seed(72)).to(DEV)
    bad = x.clone()
    bad[1, V - 1] = float("nan")                                       # a NaN in the last column
    bad[3, V // 2] = float("inf")                                      # +inf
    bad[5] = float("-inf")                                             # no finite entry
    for T, k, top_p in ((1.0, 0, 1.0), (0.5, 3, 0.9)):
        p0 = torch.empty(rows, V, dtype=torch.float32, device=DEV)
        p1 = torch.full((rows, V), 7.0, dtype=torch.float32, device=DEV)
        clean = ops.sample_rows(_wide(x), u, T, k, top_p, probs=p0)
        got = ops.sample_rows(_wide(bad), u, T, k, top_p, probs=p1)
        assert got[[1, 3, 5]].tolist() == [-1, -1, -1] and int(clean.min()) >= 0
        assert torch.equal(got[[0, 2, 4, 6]], clean[[0, 2, 4, 6]]) and torch.equal(p1[[0, 2, 4, 6]], p0[[0, 2, 4, 6]])
        assert float(p1[[1, 3, 5]].abs().max()) == 0.0                 # zeros, not what the buffer held


# ---- generate ------------------------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def _model(name, dt=torch.float32):
    kw, lc, seed, x, am, pos, _, _ = C.case_inputs(name)
    key = (name, dt)
    if key not in _MODELS:
        m = SetokimLlamaPrefill(kw)
        m.load_state_dict(O.init_llama_weights(lc, seed=seed), strict=True)
        _MODELS[key] = m.to(device=DEV, dtype=dt).eval()
    return _MODELS[key], x.to(DEV), am.to(DEV), pos.to(DEV)


def _u(n, B, seed):
    return torch.rand(n, B, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("name", ["tiny_left", "gqa_tiny_left", "dh128"])
def test_generate_with_top_k_1_is_greedy_and_sampler_none_is_todays_path(golden_dir, name):
    m, x, am, pos = _model(name)
    z = golden_io.load(os.path.join(golden_dir, "generate.npz"))
    tokens = torch.from_numpy(z[name + ":tokens"])                     # HF's greedy ids; the golden margins exclude ties
    n, B = tokens.shape
    kw = dict(inputs_embeds=x, attention_mask=am, position_ids=pos, max_new_tokens=n)
    plain = m.generate(**kw)
    assert torch.equal(plain.cpu(), tokens.t())
    assert torch.equal(m.generate(sampler=None, **kw), plain)
    for T in (1.0, 0.1):
        assert torch.equal(m.generate(sampler=Sampler(temperature=T, top_k=1, u=_u(n, B, 5)), **kw), plain)
    a = m.generate(sampler=None, return_dict_in_generate=True, output_logits=True, output_hidden_states=True, **kw)
    b = m.generate(return_dict_in_generate=True, output_logits=True, output_hidden_states=True, **kw)
    assert torch.equal(a.sequences, b.sequences) and torch.equal(a.logits, b.logits) and torch.equal(a.hidden_states, b.hidden_states)


@pytest.mark.parametrize("name,dt,kv", [("tiny_left", torch.float32, "native"), ("dh128_left", torch.bfloat16, "native"),
                                        ("dh128_left", torch.bfloat16, "fp8"), ("gqa_dh128", torch.float16, "fp8")])
def test_every_sampled_token_lies_in_the_cdf_interval_of_its_u(name, dt, kv):
    """T = 0.8, top_k = 5, top_p = 0.9 with given u and output_logits: from the returned logits of every step the fp64 rule gives each token's CDF
    interval, and the emitted token's interval contains its u within 1e-4 (the CDF error is the probability error, ~1e-6; an indexing bug misses by
    a whole interval)."""
    m, x, am, pos = _model(name, dt)
    B, n = x.shape[0], 12
    T, k, top_p = 0.8, 5, 0.9
    u = _u(n, B, 7)
    out = m.generate(inputs_embeds=x, attention_mask=am, position_ids=pos, max_new_tokens=n, kv_cache=kv, return_dict_in_generate=True,
                     output_logits=True, output_hidden_states=True, sampler=Sampler(temperature=T, top_k=k, top_p=top_p, u=u))
    assert out.sequences.shape == (B, n) and out.logits.shape[:2] == (B, n) and out.hidden_states.shape[:2] == (B, n)
    seq, lg = out.sequences.cpu(), out.logits.float().cpu()
    for b in range(B):
        for j in range(n):
            s = S.scores(lg[b, j], T)
            lo, hi = S.intervals(S.softmax_over(s, S.keep_rule(s, k, top_p)))
            t = int(seq[b, j])
            assert hi[t] > lo[t] and lo[t] - 1e-4 <= float(u[j, b]) <= hi[t] + 1e-4, (b, j, t, lo[t], float(u[j, b]), hi[t])
    again = m.generate(inputs_embeds=x, attention_mask=am, position_ids=pos, max_new_tokens=n, kv_cache=kv,
                       sampler=Sampler(temperature=T, top_k=k, top_p=top_p, u=u))
    assert torch.equal(again, out.sequences)                           # the uniforms decide the run


def test_a_generator_seed_decides_the_run():
    m, x, am, pos = _model("dh128_left", torch.bfloat16)
    kw = dict(inputs_embeds=x, attention_mask=am, position_ids=pos, max_new_tokens=16)
    run = lambda seed: m.generate(sampler=Sampler(temperature=1.5, generator=torch.Generator(device=DEV).manual_seed(seed)), **kw)
    a, b, c = run(3), run(3), run(4)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert int(a.min()) >= 0 and int(a.max()) < 128
    d = m.generate(sampler=Sampler(temperature=1.5), **kw)              # the device's default generator
    assert d.shape == a.shape and int(d.min()) >= 0


def _expected_with_eos(free, eos, pad):
    """free (B, n), the run without eos -> ((B, n') as generate must return it with the eos ids, every sequence's first eos step or n)."""
    B, n = free.shape
    exp = free.clone()
    first = []
    for b in range(B):
        first.append(next((j for j in range(n) if int(free[b, j]) in eos), n))
        exp[b, first[-1] + 1:] = pad
    return exp[:, :max(first) + 1 if max(first) < n else n], first


def test_eos_and_pad_behave_as_in_greedy():
    """A finished sequence emits pad from then on, the others' tokens are those of the run without eos (a row's uniforms do not depend on its
    neighbours: one is consumed per row per step, finished or not), and the loop ends with the step at which the last sequence finishes."""
    m, x, am, pos = _model("tiny_left")
    B, n = x.shape[0], 16
    u = _u(n, B, 9)
    kw = dict(inputs_embeds=x, attention_mask=am, position_ids=pos, max_new_tokens=n)
    free = m.generate(sampler=Sampler(temperature=1.2, top_k=20, u=u), **kw).cpu()
    b = next(b for b in range(B) if int(free[b, 3]) not in free[b, :3].tolist())
    eos, pad = int(free[b, 3]), 99
    got = m.generate(sampler=Sampler(temperature=1.2, top_k=20, u=u), eos_token_id=eos, pad_token_id=pad, **kw).cpu()
    exp, first = _expected_with_eos(free, {eos}, pad)
    assert first[b] == 3 and torch.equal(got, exp)
    every = sorted({int(t) for t in free[:, 2]})                       # every sequence has finished by step 2: the loop ends there
    exp2, first2 = _expected_with_eos(free, set(every), every[0])
    got2 = m.generate(sampler=Sampler(temperature=1.2, top_k=20, u=u), eos_token_id=every, **kw).cpu()
    assert max(first2) <= 2 and got2.shape[1] == max(first2) + 1 and torch.equal(got2, exp2)      # (pad_token_id defaults to the first eos id)


def test_a_nan_in_lm_head_raises_naming_the_sequence_and_the_step():
    kw = dict(hidden_size=64, intermediate_size=176, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=4, vocab_size=100)
    torch.manual_seed(0)
    x = torch.randn(2, 9, 64, device=DEV)
    m = SetokimLlamaPrefill(kw).to(DEV).eval()
    good = m.generate(inputs_embeds=x, max_new_tokens=3, sampler=Sampler(u=_u(3, 2, 1)))
    assert good.shape == (2, 3) and int(good.min()) >= 0
    m.lm_head.weight.data[17, 5] = float("nan")
    with pytest.raises(RuntimeError, match=r"sequence 0 at step 0"):
        m.generate(inputs_embeds=x, max_new_tokens=3, sampler=Sampler(u=_u(3, 2, 1)))                       # checked once after the loop
    with pytest.raises(RuntimeError, match=r"sequence 0 at step 0"):
        m.generate(inputs_embeds=x, max_new_tokens=3, eos_token_id=5, sampler=Sampler(u=_u(3, 2, 1)))       # checked at the step's host read
    assert m.generate(inputs_embeds=x, max_new_tokens=2).shape == (2, 2)                                    # greedy: argmax counts a NaN as the maximum, as before


def test_hf_named_sampling_arguments_stay_refused():
    kw = dict(hidden_size=64, intermediate_size=176, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=4, vocab_size=100)
    torch.manual_seed(0)
    x = torch.randn(2, 9, 64, device=DEV)
    m = SetokimLlamaPrefill(kw).to(DEV).eval()
    with pytest.raises(NotImplementedError, match="greedy"):
        m.generate(inputs_embeds=x, max_new_tokens=2, do_sample=True)
    with pytest.raises(NotImplementedError, match="greedy"):
        m.generate(inputs_embeds=x, max_new_tokens=2, do_sample=True, sampler=Sampler())
    for k, v in (("temperature", 0.1), ("top_p", 0.9), ("top_k", 5), ("num_beams", 2)):
        with pytest.raises(NotImplementedError, match="greedy"):
            m.generate(inputs_embeds=x, max_new_tokens=2, **{k: v})
    with pytest.raises(TypeError):
        m.generate(inputs_embeds=x, max_new_tokens=2, sampler="top_p")
    with pytest.raises(ValueError):
        m.generate(inputs_embeds=x, max_new_tokens=5, sampler=Sampler(u=_u(3, 2, 1)))                       # fewer rows of u than steps
