"""Per-request sampling on the GPU.  `setok_sample_rows_each` is held, bit for bit, to `setok_sample_rows` row by row under the same scalars and to
`setok_argmax_rows` on its greedy rows; a `ContinuousBatcher` whose requests bring their own samplers emits, for every request, the tokens
`generate(sampler=Sampler(..., u=U))` - or greedy `generate` - gives that request alone.  The models, prompts, ROWS / POOL and NaN-filled pools are
tests/test_paged_gpu.py's.  `pytest -m gpu`."""
import pytest
import torch

import test_paged_gpu as P

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from setok_amd import ops
    from setok_amd.generation import ContinuousBatcher, PagedKVCache, Sampler

DEV = "cuda"
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
NAN, INF = float("nan"), float("inf")


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------------------
# (temperature, top_k, top_p) of the eight rows of one launch; rows 5 - 7 get their contents in `_logits`
ROW_PARAMS = [(0.0, 7, 0.3),        # 0 greedy (top_k and top_p are ignored), with a tie at its maximum
              (0.7, 0, 1.0),        # 1
              (1.3, 5, 1.0),        # 2
              (1.0, 0, 0.9),        # 3
              (1.0, 3, 0.5),        # 4
              (1.0, 0, 1.0),        # 5 a sampled row holding a NaN: -1
              (0.0, 0, 1.0),        # 6 a greedy row holding a NaN, plus a tie at its maximum: the NaN's index
              (0.9, 4, 0.8)]        # 7 a sampled row of all -inf: -1
GUARD = -7.0
_KERNEL = {}


def _logits(dt, V, ld):
    """(8, V) as a view of an (8, ld) buffer whose other columns hold NaN: a read past V makes a sampled row -1 and a greedy row point there."""
    x = (P._rand(8, V, seed=V) * 3.0).to(dt)
    top = x.float().amax(dim=1)
    x[0, V // 3], x[0, 2 * V // 3] = top[0] + 1.0, top[0] + 1.0        # a tie at the maximum: the lower index wins
    x[5, V // 2] = NAN
    x[6, V // 4], x[6, 3 * V // 4] = top[6] + 1.0, top[6] + 1.0
    x[6, V - 2] = NAN                                                  # ... but a NaN counts as the maximum
    x[7] = -INF
    w = torch.full((8, ld), NAN, dtype=dt)
    w[:, :V] = x
    return w.to(DEV)[:, :V]


def _params(rows):
    return (torch.tensor([p[0] for p in rows], dtype=torch.float32, device=DEV), torch.tensor([p[1] for p in rows], dtype=torch.int32, device=DEV),
            torch.tensor([p[2] for p in rows], dtype=torch.float32, device=DEV))


def _each(x, u, rows):
    """One guarded launch: (out, probs) and the guard words around both, which must come back unchanged."""
    n, V = x.shape
    out = torch.full((n + 2,), int(GUARD), dtype=torch.int64, device=DEV)
    probs = torch.full((n + 2, V + 3), GUARD, dtype=torch.float32, device=DEV)
    got = ops.sample_rows_each(x, u, *_params(rows), out=out[1:-1], probs=probs[1:-1, :V])
    assert got.data_ptr() == out[1:-1].data_ptr()
    assert out[0] == int(GUARD) and out[-1] == int(GUARD) and (probs[0] == GUARD).all() and (probs[-1] == GUARD).all() and (probs[:, V:] == GUARD).all()
    return out[1:-1].clone(), probs[1:-1, :V].clone()


def _row_by_row(x, u, rows):
    """The references: `sample_rows` under each row's scalars, `argmax_rows` (and a one-hot row) for a greedy row.  Computed once per case."""
    n, V = x.shape
    out, probs = torch.empty(n, dtype=torch.int64, device=DEV), torch.full((n, V), GUARD, dtype=torch.float32, device=DEV)
    for r, (T, k, p) in enumerate(rows):
        if T == 0.0:
            ops.argmax_rows(x[r:r + 1], out=out[r:r + 1])
            probs[r] = torch.nn.functional.one_hot(out[r], V).float()
        else:
            ops.sample_rows(x[r:r + 1], u[r:r + 1], T, k, p, out=out[r:r + 1], probs=probs[r:r + 1])
    return out, probs


def _kernel_case(dtn, V, ld):
    key = (dtn, V, ld)
    if key not in _KERNEL:
        x = _logits(DTYPES[dtn], V, ld)
        u = torch.rand(8, generator=torch.Generator().manual_seed(V + 1)).to(DEV)
        _KERNEL[key] = (x, u) + _row_by_row(x, u, ROW_PARAMS)
    return _KERNEL[key]


SHAPES = [(100, 100), (32003, 32008), (36865, 36865)]                  # ld = V + 5; the first length past the LDS-resident limit (odd: unaligned rows)


@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("V,ld", SHAPES)
def test_every_row_is_selected_under_its_own_parameters_bit_for_bit(dtn, V, ld):
    x, u, want, want_p = _kernel_case(dtn, V, ld)
    assert x.stride(0) == ld
    # the references say what the rows are: two undrawable rows, the tie's lower index, the NaN's index, and draws that are not all the argmax
    assert want[5] == -1 and want[7] == -1 and want[0] == V // 3 and want[6] == V - 2 and (want_p[5] == 0).all() and (want_p[7] == 0).all()
    assert ((want_p[1:3] > 0).sum(dim=1) >= 5).all() and (want_p[1:5].sum(dim=1) - 1).abs().max() < 1e-5
    got, got_p = _each(x, u, ROW_PARAMS)
    assert torch.equal(got, want), (got.tolist(), want.tolist())
    assert torch.equal(got_p, want_p)
    assert torch.equal(got[[0, 6]], ops.argmax_rows(x)[[0, 6]])        # the greedy rows: argmax_rows over the whole matrix, too
    assert got_p[0].sum() == 1 and got_p[0, V // 3] == 1 and got_p[6].sum() == 1 and got_p[6, V - 2] == 1
    assert torch.equal(ops.sample_rows_each(x, u, *_params(ROW_PARAMS)), want)      # without out= and probs=


@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("V,ld", SHAPES)
def test_reversing_the_rows_reverses_the_result(dtn, V, ld):
    x, u, want, want_p = _kernel_case(dtn, V, ld)
    w = torch.full((8, ld), NAN, dtype=x.dtype, device=DEV)
    w[:, :V] = x.flip(0)
    got, got_p = _each(w[:, :V], u.flip(0).contiguous(), ROW_PARAMS[::-1])
    assert torch.equal(got, want.flip(0)) and torch.equal(got_p, want_p.flip(0))


@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("V,ld", SHAPES)
def test_out_of_domain_parameters_give_minus_one_for_their_row_alone(dtn, V, ld):
    x, u, _, _ = _kernel_case(dtn, V, ld)
    x = x.clone()                                                      # rows 1 - 4 are drawable; copy them over the others so that only a parameter is bad
    x[[0, 5, 6, 7]] = x[[1, 2, 3, 4]]
    rows = [(NAN, 0, 1.0), (-1.0, 0, 1.0), (INF, 0, 1.0), (1.0, -1, 1.0), (1.0, 0, 0.0), (1.0, 0, 1.5), (0.7, 3, 0.9), (1.0, -(2 ** 31), NAN)]
    got, got_p = _each(x, u, rows)
    want6 = torch.empty(1, dtype=torch.int64, device=DEV)
    want6_p = torch.empty(1, V, dtype=torch.float32, device=DEV)
    ops.sample_rows(x[6:7], u[6:7], 0.7, 3, 0.9, out=want6, probs=want6_p)
    assert got.tolist() == [-1] * 6 + [int(want6)] + [-1] and int(want6) >= 0
    assert torch.equal(got_p[6], want6_p[0]) and (got_p[:6] == 0).all() and (got_p[7] == 0).all()


# ---- the batcher -----------------------------------------------------------------------------------------------------------------------------------
SAMPLED = {0: dict(temperature=1.5), 2: dict(temperature=0.8, top_k=20), 4: dict(temperature=1.0, top_p=0.9)}      # requests 1 and 3 stay greedy
TEMPERATURE_ONLY = {0: dict(temperature=1.5), 2: dict(temperature=0.8), 4: dict(temperature=1.0)}
_ALONE = {}


def _u(s, n):
    return torch.rand(n, 1, generator=torch.Generator().manual_seed(s))


def _alone(m, xs, news, kws, s, tag, **gen_kw):
    """The reference arm: request i alone through `generate` with its sampler on the stream U = _u(s, n) - greedy where kws has no entry.  Computed
    once per case and shared: [(tokens, logits (n', V), u or None)]."""
    key = (tag, s if kws else None, tuple((i, tuple(sorted(kw.items()))) for i, kw in sorted(kws.items())), tuple(sorted(gen_kw.items())))
    if key not in _ALONE:
        res = []
        for i, (x, n) in enumerate(zip(xs, news)):
            u = _u(s, n) if i in kws else None
            kw = dict(gen_kw, sampler=Sampler(**kws[i], u=u.clone())) if i in kws else gen_kw
            out = m.generate(inputs_embeds=x[None], max_new_tokens=n, return_dict_in_generate=True, output_logits=True, **kw)
            res.append((out.sequences[0], out.logits[0], u))
        _ALONE[key] = res
    return _ALONE[key]


def _first_seed(m, xs, news, kws, tag, **gen_kw):
    """The first stream seed in 0..5 for which the reference arms alone show that sampling happened: every sampled request's tokens differ from
    its greedy tokens somewhere."""
    greedy = _alone(m, xs, news, {}, 0, tag, **gen_kw)
    for s in range(6):
        alone = _alone(m, xs, news, kws, s, tag, **gen_kw)
        differs = all(alone[i][0].tolist() != greedy[i][0].tolist() for i in kws)
        print(f"{tag}: stream seed {s}: every sampled request differs from its greedy tokens: {differs}")
        if differs:
            return s, alone, greedy
    raise AssertionError(f"{tag}: no stream seed in 0..5 makes every sampled request differ from its greedy tokens")


def _samplers(kws, s, news):
    return {i: Sampler(**kw, u=_u(s, news[i])) for i, kw in kws.items()}


def _batcher(m, eos=None):
    b = ContinuousBatcher(m, P.ROWS, P.POOL, max_pages_per_seq=2, eos_token_id=eos)
    for t in b.cache.k + b.cache.v:
        t.fill_(float("nan"))                                          # nothing may depend on what a pool holds
    return b


def _requests(xs, news, samplers):
    return [(x, n, None, samplers.get(i)) for i, (x, n) in enumerate(zip(xs, news))]


def _tokens(res):
    return [t.tolist() for t, _, _ in res]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", list(P.CONFIGS))
def test_sampled_and_greedy_requests_share_a_batch_and_equal_each_request_alone(name, dt):
    m, xs, tag = P._model(name, dt, 5), P._prompts(name, dt, 5), f"{name} {dt}"
    s, want, greedy = _first_seed(m, xs, P.NEW, SAMPLED, tag)
    assert _tokens(greedy) == [t.tolist() for t in P._alone(name, dt, 5)[0]]         # the greedy arm is test_paged_gpu.py's
    b = _batcher(m)
    got = b.run(_requests(xs, P.NEW, _samplers(SAMPLED, s, P.NEW)))
    assert [g.tolist() for g in got] == _tokens(want) and all(torch.equal(g, w[0]) for g, w in zip(got, want))
    assert [g.numel() for g in got] == list(P.NEW) and b.errors == {}
    st = b.stats
    assert st["admitted"] == 5 and st["admitted_midflight"] >= 1 and st["page_waits"] >= 1 and st["pages_reused"] >= 1
    assert st["pages_high_water"] == P.POOL and 0 < st["row_steps_active"] <= st["row_steps_total"] == P.ROWS * st["steps"]
    assert b.cache.pages_free == P.POOL and b.cache.lens.tolist() == [0] * P.ROWS and b.cache.block_table.tolist() == [[-1, -1]] * P.ROWS
    assert b.temperature.tolist() == [0.0] * P.ROWS                                  # every row is idle: a greedy row
    eos = P._mid_sequence_eos([w[0] for w in want])
    want_e = _alone(m, xs, P.NEW, SAMPLED, s, tag, eos_token_id=eos)
    assert any(w[0].numel() < n for w, n in zip(want_e, P.NEW)) and all(int(w[0][-1]) == eos or w[0].numel() == n for w, n in zip(want_e, P.NEW))
    b = _batcher(m, eos)
    got_e = b.run(_requests(xs, P.NEW, _samplers(SAMPLED, s, P.NEW)))
    assert [g.tolist() for g in got_e] == _tokens(want_e) and b.cache.pages_free == P.POOL


def _cdf_margin(alone, kws):
    """The smallest distance of any draw's uniform from the edges of its token's interval of the index-order CDF, the distribution taken from
    `sample_rows` on the alone arm's own logits row."""
    return min(_draw_margin(*alone[i], kw["temperature"]) for i, kw in kws.items())


def _draw_margin(toks, logits, u, temperature):
    """One request's draws (row j of the logits drew token j with u[j, 0]): all rows share the temperature, so one `sample_rows` launch."""
    n, V = logits.shape
    probs = torch.empty(n, V, dtype=torch.float32, device=DEV)
    ud = u[:n, 0].to(DEV)
    tok = ops.sample_rows(logits.contiguous(), ud.contiguous(), temperature, 0, 1.0, probs=probs)
    assert torch.equal(tok, toks)
    hi = probs.double().cumsum(1).gather(1, tok[:, None])[:, 0]
    lo = hi - probs.double().gather(1, tok[:, None])[:, 0]
    return float(torch.minimum(ud.double() - lo, hi - ud.double()).min())


# fp32: the model seeds of test_paged_gpu.py's tiny Llamas under which the reference arms ALONE meet both preconditions of the test below.  These
# 100-token models' distributions are nearly flat - every interval of the CDF is about 0.01 wide - so a draw lies within MIN_MARGIN = 1e-3 of one
# of its own two edges with probability about 0.2, and all 25 draws keep clear under a given stream in about 1 model in 250: test_paged_gpu.py's
# seeds 5..10 have no such stream among 0..5 (smallest margins 1.0e-4 ... 6.1e-4 for dh16 at seed 6, 9.6e-7 ... 1.7e-4 for dh128 at seed 5).  A scan
# of the model seeds 5, 6, 7, ... that ran the reference arms only - `generate` and `sample_rows`, never the batcher - found, up to seed 181,
# dh16: 82 (stream 5, margin 1.006e-3), 156 (stream 3, 1.164e-3), 180 (stream 1, 1.071e-3); dh128: 55 (stream 5, 1.326e-3; its greedy top-2 margin
# fails), 78 (stream 0, 1.007e-3), 179 (stream 0, 1.086e-3).  Recorded here: the seed of each config with the most room; the test asserts the
# preconditions on it and does not repeat the scan.
FP32_MODEL_SEED = {"dh16": 156, "dh128": 179}


@pytest.mark.parametrize("name", list(P.CONFIGS))
def test_sampled_and_greedy_requests_equal_each_request_alone_in_fp32(name):
    """fp32 logits are not bit-identical between one row and several, so no selection may sit on an edge.  Preconditions, on the reference arms
    alone: the model's greedy selections keep test_paged_gpu.py's top-2 margin (its own rule and arm; requests 1 and 3 stay greedy here, 13
    selections), and a stream seed in 0..5 - the first is taken - makes every sampled request differ from its greedy tokens and keeps every one
    of its 25 draws at least MIN_MARGIN inside its token's interval of the index-order CDF: 38 guarded selections in all.  1e-3 is orders of
    magnitude above what an fp32 summation order can move a CDF edge.  Temperature-only samplers.  Then the tokens are equal."""
    dt, seed = torch.float32, FP32_MODEL_SEED[name]
    _, margin = P._alone(name, dt, seed)
    print(f"{name} fp32 model seed {seed}: smallest top-2 margin of the greedy alone runs {margin:.3e}")
    assert margin >= P.MIN_MARGIN
    m, xs, tag = P._model(name, dt, seed), P._prompts(name, dt, seed), f"{name} fp32 model seed {seed}"
    greedy = _alone(m, xs, P.NEW, {}, 0, tag)
    want = None
    for s in range(6):
        alone = _alone(m, xs, P.NEW, TEMPERATURE_ONLY, s, tag)
        differs = all(alone[i][0].tolist() != greedy[i][0].tolist() for i in TEMPERATURE_ONLY)
        cdf_margin = _cdf_margin(alone, TEMPERATURE_ONLY)
        print(f"{tag}: stream seed {s}: sampled requests differ from greedy: {differs}; smallest CDF margin of the 25 draws {cdf_margin:.3e}")
        if differs and cdf_margin >= P.MIN_MARGIN:
            want = alone
            break
    assert want is not None, "no stream seed in 0..5 keeps every draw MIN_MARGIN inside its CDF interval"
    assert sum(w[0].numel() for w in want) == 38
    got = _batcher(m).run(_requests(xs, P.NEW, _samplers(TEMPERATURE_ONLY, s, P.NEW)))
    assert [g.tolist() for g in got] == _tokens(want)


PREFIX_ROWS = 140                                                      # one shared page and a tail of 12 rows
REQUESTS_P = ((True, 3, 6, dict(temperature=1.5)), (True, 40, 5, None), (False, 50, 7, dict(temperature=0.8, top_k=20)),
              (True, 100, 4, dict(temperature=1.0, top_p=0.9)))       # (behind the prefix?, remainder rows, max_new_tokens, sampler)


def test_a_sampled_request_behind_a_shared_prefix_draws_its_first_token_with_u0():
    name, dt = "dh16", torch.bfloat16
    m, D = P._model(name, dt, 5), P.CONFIGS[name]["hidden_size"]
    prefix = P._rand(PREFIX_ROWS, D, seed=5090).to(dt).to(DEV)
    rest = [P._rand(S, D, seed=5100 + i).to(dt).to(DEV) for i, (_, S, _, _) in enumerate(REQUESTS_P)]
    want, differs = [], []
    for (pre, _, n, kw), x in zip(REQUESTS_P, rest):
        full, gen_kw = (torch.cat([prefix, x]), dict(prefill_chunk=P.PAGE)) if pre else (x, {})
        arms = [m.generate(inputs_embeds=full[None], max_new_tokens=n, **gen_kw, **extra)[0]
                for extra in ([{}] if kw is None else [dict(sampler=Sampler(**kw, u=_u(3, n))), {}])]
        want.append(arms[0])
        differs.append(kw is None or arms[0].tolist() != arms[1].tolist())
    assert all(differs)                                                # the reference arms alone show that sampling happened
    pool = 4
    b = ContinuousBatcher(m, 2, pool, max_pages_per_seq=3)
    for t in b.cache.k + b.cache.v:
        t.fill_(float("nan"))
    h = b.register_prefix(prefix)
    got = b.run([(x, n, h if pre else None, None if kw is None else Sampler(**kw, u=_u(3, n))) for (pre, _, n, kw), x in zip(REQUESTS_P, rest)])
    assert [g.tolist() for g in got] == [w.tolist() for w in want]
    assert b.prefix_stats == dict(registered=1, hits=3, slots_shared=3 * 128) and b.cache.pages_free == pool - 1
    b.drop_prefix(h)
    assert b.cache.pages_free == pool and b.cache.page_refs == [0] * pool


def test_sampled_requests_over_mxfp4_pages_equal_generate_over_the_mxfp4_cache():
    name, dt = "dh128", torch.bfloat16
    m, xs, tag = P._model(name, dt, 5), P._prompts(name, dt, 5), "dh128 bf16 mxfp4 pages"
    s, want, _ = _first_seed(m, xs, P.NEW, SAMPLED, tag, kv_cache="mxfp4")
    cache = PagedKVCache.for_model(m.model, P.ROWS, P.POOL, 2, kv_format="mxfp4")
    for layers in (cache.k_q, cache.k_s, cache.v_q, cache.v_s):
        for t in layers:
            t.fill_(0xFF)                                              # every unwritten block is a NaN block
    b = ContinuousBatcher(m, P.ROWS, cache=cache)
    got = b.run(_requests(xs, P.NEW, _samplers(SAMPLED, s, P.NEW)))
    assert [g.tolist() for g in got] == _tokens(want) and cache.pages_free == P.POOL and b.stats["page_waits"] >= 1


def test_all_greedy_submissions_never_make_the_per_row_launch(monkeypatch):
    name, dt = "dh16", torch.bfloat16
    m, xs = P._model(name, dt, 5), P._prompts(name, dt, 5)

    def boom(*a, **k):
        raise AssertionError("an all-greedy batch called sample_rows_each")
    monkeypatch.setattr(ops, "sample_rows_each", boom)
    monkeypatch.setattr(ops, "sample_rows", boom)
    got = _batcher(m).run(_requests(xs, P.NEW, {}))
    assert [g.tolist() for g in got] == [w.tolist() for w in P._alone(name, dt, 5)[0]]


def test_a_mixed_step_makes_one_per_row_launch_and_no_argmax(monkeypatch):
    name, dt = "dh16", torch.bfloat16
    m, xs, tag = P._model(name, dt, 5), P._prompts(name, dt, 5), f"{name} {dt}"
    s, want, _ = _first_seed(m, xs, P.NEW, SAMPLED, tag)
    b = _batcher(m)
    each, argmax, scalar = [], [], []
    real_each, real_argmax, real_scalar = ops.sample_rows_each, ops.argmax_rows, ops.sample_rows
    monkeypatch.setattr(ops, "sample_rows_each", lambda x, *a, **k: (each.append((b.stats["steps"], x.shape[0])), real_each(x, *a, **k))[1])
    monkeypatch.setattr(ops, "argmax_rows", lambda x, *a, **k: (argmax.append((b.stats["steps"], x.shape[0])), real_argmax(x, *a, **k))[1])
    monkeypatch.setattr(ops, "sample_rows", lambda x, *a, **k: (scalar.append((b.stats["steps"], x.shape[0])), real_scalar(x, *a, **k))[1])
    got = b.run(_requests(xs, P.NEW, _samplers(SAMPLED, s, P.NEW)))
    assert [g.tolist() for g in got] == _tokens(want)
    steps_each = [t for t, _ in each]
    steps_argmax = [t for t, rows in argmax if rows == P.ROWS]         # a one-row call is an admission's
    assert all(rows == P.ROWS for _, rows in each) and len(set(steps_each)) == len(steps_each) >= 1      # at most one per step
    assert not set(steps_each) & set(steps_argmax) and len(set(steps_argmax)) == len(steps_argmax)
    assert sorted(steps_each + steps_argmax) == list(range(b.stats["steps"]))                            # every step selected exactly once
    assert len(scalar) == 3 and len([1 for _, rows in argmax if rows == 1]) == 2                         # the admissions: one row each


def test_an_undrawable_request_ends_alone_and_the_others_are_unaffected():
    """Request 2's prompt embeddings hold a NaN: every state of it is NaN, so its first selection already fails."""
    name, dt = "dh16", torch.bfloat16
    m, xs, tag = P._model(name, dt, 5), list(P._prompts(name, dt, 5)), f"{name} {dt}"
    s, want, _ = _first_seed(m, xs, P.NEW, SAMPLED, tag)
    xs[2] = xs[2].clone()
    xs[2][0, 0] = NAN
    b = _batcher(m)
    tickets = [b.submit(x, n, sampler=sm) for x, n, _, sm in _requests(xs, P.NEW, _samplers(SAMPLED, s, P.NEW))]
    out = {}
    while b.queue or any(r is not None for r in b.running):
        out.update(b.step())
    bad = tickets[2]
    assert out[bad].numel() == 0 and out[bad].dtype == torch.int64 and list(b.errors) == [bad]
    assert f"request {bad} at step 0" in b.errors[bad] and "NaN or +inf, or no finite entry: no token can be drawn" in b.errors[bad]
    for i, t in enumerate(tickets):
        if i != 2:
            assert out[t].tolist() == want[i][0].tolist(), i
    assert b.cache.pages_free == P.POOL and b.cache.lens.tolist() == [0] * P.ROWS and b.cache.block_table.tolist() == [[-1, -1]] * P.ROWS
    assert b.temperature.tolist() == [0.0] * P.ROWS
    b = _batcher(m)
    with pytest.raises(RuntimeError, match=rf"tickets \[{bad}\]"):
        b.run(_requests(xs, P.NEW, _samplers(SAMPLED, s, P.NEW)))
    assert not b.queue and all(r is None for r in b.running) and b.cache.pages_free == P.POOL and b.stats["admitted"] == 5      # drained first
