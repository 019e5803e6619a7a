"""Per-request sampling in the continuous batcher, without a GPU: setok_sample_rows_each is declared, exported by both builds and mirrored by the
ctypes table; it refuses bad arguments on the host before any launch; `ContinuousBatcher.submit(sampler=)` validates and leaves no trace; and the
scheduler - on test_paged_cpu.py's scripted model, with torch stand-ins for the selection ops - draws every request from its own stream, makes one
selection call per step, keeps the greedy step's calls, and ends an undrawable request without touching the others."""
import ctypes
import inspect
import os
import re
import sys

import pytest
import torch

from test_paged_cpu import D, _prompt, _scripted_batcher

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, ARITY = "setok_sample_rows_each", 13


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    from setok_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH) or not os.path.isfile(_lib.LIB_PATH_F16):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_the_entry_is_declared_exported_and_in_the_ctypes_table(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "setok_hip.h")).read(), flags=re.S)
    decls = {n: [a for a in args.split(",") if a.strip()] for n, args in re.findall(r"\bint\s+(setok_\w+)\s*\(([^;]*)\)\s*;", text, flags=re.S)}
    assert NAME in decls and len(decls[NAME]) == ARITY
    assert NAME in lib.SIGNATURES and len(lib.SIGNATURES[NAME]) == ARITY
    for path in (lib.LIB_PATH, lib.LIB_PATH_F16):
        assert hasattr(ctypes.CDLL(path), NAME), f"{NAME} not exported by {os.path.basename(path)}"
    assert lib.load().setok_abi_version() == 9 and lib.load(half=True).setok_abi_version() == 9      # additive: the ABI version stays


@pytest.mark.parametrize("half", [False, True])
def test_bad_arguments_are_refused_on_the_host(lib, half):
    l = lib.load(half)
    P = 64                                                            # a non-null "pointer": validation fails before anything is dereferenced
    # setok_sample_rows_each(stream, dtype, logits, ld, rows, V, u, temperature, top_k, top_p, out, probs, ld_probs)
    bad = [
        ((None, 0, None, 8, 1, 8, P, P, P, P, P, None, 0), b"null operand"),                     # logits
        ((None, 0, P, 8, 1, 8, None, P, P, P, P, None, 0), b"null operand"),                     # u
        ((None, 0, P, 8, 1, 8, P, None, P, P, P, None, 0), b"null operand"),                     # temperature
        ((None, 0, P, 8, 1, 8, P, P, None, P, P, None, 0), b"null operand"),                     # top_k
        ((None, 0, P, 8, 1, 8, P, P, P, None, P, None, 0), b"null operand"),                     # top_p
        ((None, 0, P, 8, 1, 8, P, P, P, P, None, None, 0), b"null operand"),                     # out
        ((None, 0, P, 8, 0, 8, P, None, P, P, P, None, 0), b"null operand"),                     # ... also with nothing to do
        ((None, 0, P, 8, 1, 0, P, P, P, P, P, None, 0), b"bad shape"),                           # V < 1
        ((None, 0, P, 1 << 21, 1, (1 << 20) + 1, P, P, P, P, P, None, 0), b"bad shape"),         # V > 2^20
        ((None, 0, P, 7, 1, 8, P, P, P, P, P, None, 0), b"bad shape"),                           # ld < V
        ((None, 0, P, 8, 1, 8, P, P, P, P, P, P, 7), b"bad shape"),                              # ld_probs < V with probs
        ((None, 0, P, 8, -1, 8, P, P, P, P, P, None, 0), b"bad shape"),                          # rows < 0
        ((None, 7, P, 8, 1, 8, P, P, P, P, P, None, 0), b"bad dtype"),
        ((None, 2 if not half else 1, P, 8, 1, 8, P, P, P, P, P, None, 0), b"bad dtype"),        # the other build's 16-bit type
        ((None, 7, P, 8, 0, 8, P, P, P, P, P, None, 0), b"bad dtype"),                           # ... also with nothing to do
    ]
    for args, msg in bad:
        rc = l.setok_sample_rows_each(*args)
        err = l.setok_last_error()
        assert rc == -1 and msg in err and b"setok_sample_rows_each" in err, (args, err)
    for dt in (0, 2 if half else 1):                                  # nothing to do is not an error (and launches nothing)
        assert l.setok_sample_rows_each(None, dt, P, 8, 0, 8, P, P, P, P, P, None, 0) == 0
        assert l.setok_sample_rows_each(None, dt, P, 8, 0, 8, P, P, P, P, P, P, 8) == 0


def test_submit_and_ops_carry_the_surface(lib):
    from setok_amd import ops
    from setok_amd.generation import ContinuousBatcher
    sig = inspect.signature(ContinuousBatcher.submit)
    assert sig.parameters["sampler"].default is None and list(sig.parameters)[-1] == "sampler"
    assert list(inspect.signature(ops.sample_rows_each).parameters) == ["logits", "u", "temperature", "top_k", "top_p", "out", "probs"]
    assert "submit(sampler=)" in ContinuousBatcher.__doc__ or "submit(..., sampler=" in ContinuousBatcher.__doc__


def test_submit_validates_the_sampler_and_leaves_no_trace_and_the_constructor_still_refuses(monkeypatch):
    from setok_amd.generation import ContinuousBatcher, Sampler
    b, _ = _scripted_batcher(monkeypatch, {}, rows=2, num_pages=3, max_pages_per_seq=2)
    table, lens = b.cache.block_table.clone(), b.cache.lens.clone()
    for bad in (0.7, dict(temperature=0.7), "greedy", torch.rand(4, 1), Sampler):
        with pytest.raises(TypeError, match="ContinuousBatcher.submit: sampler="):
            b.submit(_prompt(0, 3), 4, sampler=bad)
    for u in (torch.rand(3, 1), torch.rand(4, 2), torch.rand(8, 0)):   # too few steps; a batch-wide stream; no column
        with pytest.raises(ValueError, match="ContinuousBatcher.submit: the sampler's u"):
            b.submit(_prompt(0, 3), 4, sampler=Sampler(u=u))
    assert b.queue == [] and b._tickets == 0 and b.cache.pages_free == 3 and b.cache.table_host == [[-1, -1]] * 2
    assert torch.equal(b.cache.block_table, table) and torch.equal(b.cache.lens, lens) and b.errors == {}
    assert b.submit(_prompt(0, 3), 4, sampler=Sampler(u=torch.rand(4, 1))) == 0 and b.submit(_prompt(1, 3), 4, sampler=Sampler(u=torch.rand(9, 1))) == 1
    assert b.submit(_prompt(2, 3), 4, sampler=Sampler(0.5, 3, 0.9, generator=torch.Generator().manual_seed(1))) == 2 and len(b.queue) == 3
    with pytest.raises(NotImplementedError, match="sampler=") as e:
        ContinuousBatcher(b.lm, 2, 3, sampler=Sampler())
    assert "submit(" in str(e.value)                                  # the reason points at where a sampler goes


# ---- the scheduler, with torch stand-ins for the two sampling ops --------------------------------------------------------------------------------
def _draw(logits, u, T, k, p):
    """A stand-in with the ops' contract on the scripted one-hot rows: greedy at T == 0, -1 for a row with a NaN; a sampled row takes the argmax
    when u < 0.5 and the token 59 - argmax otherwise, so a stream shows in the tokens."""
    out = []
    for r in range(logits.shape[0]):
        t = float(T[r]) if isinstance(T, torch.Tensor) else T
        top = int(logits[r].argmax())
        if t == 0.0:
            out.append(top)
        elif bool(torch.isnan(logits[r]).any()):
            out.append(-1)
        else:
            out.append(top if float(u.reshape(-1)[r]) < 0.5 else 59 - top)
    return torch.tensor(out, dtype=torch.int64)


def _sampling_batcher(monkeypatch, scripts, **kw):
    from setok_amd import ops
    b, log = _scripted_batcher(monkeypatch, scripts, **kw)
    calls = []
    monkeypatch.setattr(ops, "argmax_rows", lambda x, out=None: (calls.append(("argmax", x.shape[0], b.stats["steps"])), x.argmax(-1))[1])

    def sample_rows(logits, u, temperature=1.0, top_k=0, top_p=1.0, out=None, probs=None):
        calls.append(("scalar", logits.shape[0], b.stats["steps"], (temperature, top_k, top_p), float(u)))
        return _draw(logits, u, temperature, top_k, top_p)

    def sample_rows_each(logits, u, temperature, top_k, top_p, out=None, probs=None):
        assert u.shape == temperature.shape == top_k.shape == top_p.shape == (logits.shape[0],)
        assert (temperature.dtype, top_k.dtype, top_p.dtype, u.dtype) == (torch.float32, torch.int32, torch.float32, torch.float32)
        calls.append(("each", logits.shape[0], b.stats["steps"], temperature.tolist(), top_k.tolist(), [round(x, 6) for x in top_p.tolist()], u.tolist()))
        return _draw(logits, u, temperature, top_k, top_p)

    monkeypatch.setattr(ops, "sample_rows", sample_rows)
    monkeypatch.setattr(ops, "sample_rows_each", sample_rows_each)
    return b, log, calls


SHAPES = [(100, 6), (10, 3), (5, 4), (20, 1), (5, 5)]                 # (prompt rows, max_new_tokens)
SCRIPTS = [[(7 * i + j) % 50 + 1 for j in range(n + 1)] for i, (_, n) in enumerate(SHAPES)]


def _expected(script, n, u):
    """The scripted model does not look at what it is fed, so request i's tokens are its script, flipped where its own u says so."""
    return [t if u is None or float(u[j, 0]) < 0.5 else 59 - t for j, t in enumerate(script[:n])]


def test_every_request_draws_from_its_own_stream_with_one_selection_call_per_step(monkeypatch):
    from setok_amd.generation import Sampler
    b, log, calls = _sampling_batcher(monkeypatch, SCRIPTS, rows=2, num_pages=3, max_pages_per_seq=2)
    us = {i: torch.rand(n + 2, 1, generator=torch.Generator().manual_seed(10 + i)) for i, (_, n) in enumerate(SHAPES) if i in (0, 2, 3)}
    params = {0: (1.5, 0, 1.0), 2: (0.8, 20, 1.0), 3: (1.0, 0, 0.9)}
    reqs = [(_prompt(i, T), n, None, Sampler(*params[i], u=us[i]) if i in us else None) for i, (T, n) in enumerate(SHAPES)]
    got = b.run(reqs)
    assert [g.tolist() for g in got] == [_expected(SCRIPTS[i], n, us.get(i)) for i, (_, n) in enumerate(SHAPES)]
    assert any(g.tolist() != SCRIPTS[i][:n] for i, ((_, n), g) in enumerate(zip(SHAPES, got)) if i in us)      # a stream showed
    assert b.errors == {} and b.cache.pages_free == 3 and b.temperature.tolist() == [0.0, 0.0]
    # admissions: one row each, argmax for a greedy request, the scalar launch with u[0] for a sampled one
    firsts = [c for c in calls if c[1] == 1]
    assert [c[0] for c in firsts] == ["scalar", "argmax", "scalar", "scalar", "argmax"]
    assert [(c[3], c[4]) for c in firsts if c[0] == "scalar"] == [(params[i], float(us[i][0, 0])) for i in (0, 2, 3)]
    # decode steps: exactly one selection call over both rows per step; the per-row launch iff a sampled row decodes in it
    steps = [c for c in calls if c[1] == 2]
    assert [c[2] for c in steps] == list(range(b.stats["steps"]))
    for c, flags in zip(steps, log["decodes"]):
        if c[0] == "each":
            assert any(t > 0 for t, f in zip(c[3], flags) if f)        # a sampled row decodes in it
    # rows (request 0: T = 1.5, request 1: greedy) in steps 0 and 1; request 2 (T = 0.8, k = 20) takes row 1 in step 2 with its u[1]
    assert steps[0][3:6] == ([1.5, 0.0], [0, 0], [1.0, 1.0]) and steps[0][6][0] == float(us[0][1, 0])
    assert steps[2][4] == [0, 20] and steps[2][6] == [float(us[0][3, 0]), float(us[2][1, 0])]
    # requests 3 (one token: its admission's) and 4 (greedy) come last: no sampled row decodes, so the steps call argmax_rows as before
    assert [c[0] for c in steps] == ["each"] * 5 + ["argmax"] * 4


def test_all_greedy_submissions_never_touch_the_sampling_ops(monkeypatch):
    from setok_amd import ops
    b, log, calls = _sampling_batcher(monkeypatch, SCRIPTS, rows=2, num_pages=3, max_pages_per_seq=2)

    def boom(*a, **k):
        raise AssertionError("a greedy batch called a sampling op")
    monkeypatch.setattr(ops, "sample_rows", boom)
    monkeypatch.setattr(ops, "sample_rows_each", boom)
    got = b.run([(_prompt(i, T), n) for i, (T, n) in enumerate(SHAPES)])
    assert [g.tolist() for g in got] == [SCRIPTS[i][:n] for i, (_, n) in enumerate(SHAPES)]
    assert {c[0] for c in calls} == {"argmax"} and len([c for c in calls if c[1] == 2]) == b.stats["steps"]


def test_a_generator_stream_is_one_draw_of_max_new_tokens_at_admission(monkeypatch):
    from setok_amd.generation import Sampler
    b, log, calls = _sampling_batcher(monkeypatch, SCRIPTS, rows=2, num_pages=3, max_pages_per_seq=2)
    g = torch.Generator().manual_seed(77)
    got = b.run([(_prompt(0, 100), 6, None, Sampler(generator=g)), (_prompt(1, 10), 3)])
    g2 = torch.Generator().manual_seed(77)
    u = torch.rand((6, 1), generator=g2)
    assert got[0].tolist() == _expected(SCRIPTS[0], 6, u) and got[1].tolist() == SCRIPTS[1][:3]
    assert torch.equal(torch.rand(3, generator=g), torch.rand(3, generator=g2))          # that one draw is all the request consumed


@pytest.mark.parametrize("bad_at", [0, 2])
def test_an_undrawable_request_ends_alone_and_run_raises_after_draining(monkeypatch, bad_at):
    """Request 2's state turns NaN at its token `bad_at` (0: the admission's selection): it ends there with the tokens before, an `errors` entry
    and its pages back; the others finish with their own tokens."""
    from setok_amd import ops
    from setok_amd.generation import Sampler
    us = {i: torch.rand(n, 1, generator=torch.Generator().manual_seed(20 + i)) for i, (_, n) in enumerate(SHAPES) if i in (0, 2)}
    reqs = [(_prompt(i, T), n, None, Sampler(u=us[i]) if i in us else None) for i, (T, n) in enumerate(SHAPES)]

    def poisoned(monkeypatch):
        b, log, calls = _sampling_batcher(monkeypatch, SCRIPTS, rows=2, num_pages=3, max_pages_per_seq=2)
        linear = ops.linear

        def nan_linear(a, w, **kw):                                    # the scripted state of request 2's token `bad_at` is one-hot(SCRIPTS[2][bad_at])
            y = linear(a, w, **kw).clone()
            y[y.argmax(-1) == SCRIPTS[2][bad_at]] = float("nan")
            return y
        monkeypatch.setattr(ops, "linear", nan_linear)
        return b
    assert all(SCRIPTS[2][bad_at] not in s[:n] for i, ((_, n), s) in enumerate(zip(SHAPES, SCRIPTS)) if i != 2)      # only request 2 has that state
    b = poisoned(monkeypatch)
    tickets = [b.submit(r[0], r[1], sampler=r[3]) for r in reqs]
    out = {}
    while b.queue or any(r is not None for r in b.running):
        done = b.step()
        if 2 in dict(done):                                            # released in the step it failed in
            assert b.cache.pages_free >= 1 and 2 in b.errors
        out.update(done)
    assert out[2].dtype == torch.int64 and out[2].tolist() == _expected(SCRIPTS[2], bad_at, us[2])
    assert list(b.errors) == [2] and f"request 2 at step {bad_at}" in b.errors[2] and "no token can be drawn" in b.errors[2]
    for i, (_, n) in enumerate(SHAPES):
        if i != 2:
            assert out[i].tolist() == _expected(SCRIPTS[i], n, us.get(i))
    assert b.cache.pages_free == 3 and b.cache.table_host == [[-1, -1]] * 2 and b.temperature.tolist() == [0.0, 0.0]
    b = poisoned(monkeypatch)
    with pytest.raises(RuntimeError, match=r"ContinuousBatcher.run: the requests with tickets \[2\]"):
        b.run(reqs)
    assert not b.queue and all(r is None for r in b.running) and b.cache.pages_free == 3 and b.stats["admitted"] == len(SHAPES)      # drained first
