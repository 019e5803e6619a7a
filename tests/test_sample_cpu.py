"""Sampled token selection, without a GPU: setok_sample_rows is declared, exported by both builds and mirrored by the ctypes table; it refuses bad
arguments on the host before any launch; generation.Sampler validates like it; generate() carries `sampler=None`; and the committed fixture
tests/golden/sample.npz (HuggingFace's three logits warpers, tests/golden/make_golden_sample.py) has the shapes, the kept sets and the margins the
GPU tests rely on."""
import ctypes
import inspect
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import golden_io
import sample_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, ARITY = "setok_sample_rows", 13


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    from setok_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH) or not os.path.isfile(_lib.LIB_PATH_F16):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


@pytest.fixture(scope="module")
def golden(golden_dir):
    return golden_io.load(os.path.join(golden_dir, "sample.npz"))


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
    nan, inf = float("nan"), float("inf")
    # setok_sample_rows(stream, dtype, logits, ld, rows, V, u, temperature, top_k, top_p, out, probs, ld_probs)
    bad = [
        ((None, 0, None, 8, 1, 8, P, 1.0, 0, 1.0, P, None, 0), b"null operand"),                 # logits
        ((None, 0, P, 8, 1, 8, None, 1.0, 0, 1.0, P, None, 0), b"null operand"),                 # u
        ((None, 0, P, 8, 1, 8, P, 1.0, 0, 1.0, None, None, 0), b"null operand"),                 # out
        ((None, 0, P, 8, 1, 0, P, 1.0, 0, 1.0, P, None, 0), b"bad shape"),                       # V < 1
        ((None, 0, P, 1 << 21, 1, (1 << 20) + 1, P, 1.0, 0, 1.0, P, None, 0), b"bad shape"),     # V > 2^20
        ((None, 0, P, 7, 1, 8, P, 1.0, 0, 1.0, P, None, 0), b"bad shape"),                       # ld < V
        ((None, 0, P, 8, 1, 8, P, 1.0, 0, 1.0, P, P, 7), b"bad shape"),                          # ld_probs < V with probs
        ((None, 0, P, 8, -1, 8, P, 1.0, 0, 1.0, P, None, 0), b"bad shape"),                      # rows < 0
        ((None, 0, P, 8, 1, 8, P, 0.0, 0, 1.0, P, None, 0), b"bad temperature"),
        ((None, 0, P, 8, 1, 8, P, -1.0, 0, 1.0, P, None, 0), b"bad temperature"),
        ((None, 0, P, 8, 1, 8, P, nan, 0, 1.0, P, None, 0), b"bad temperature"),
        ((None, 0, P, 8, 1, 8, P, inf, 0, 1.0, P, None, 0), b"bad temperature"),
        ((None, 0, P, 8, 1, 8, P, 1.0, -1, 1.0, P, None, 0), b"bad top_k"),
        ((None, 0, P, 8, 1, 8, P, 1.0, 0, 0.0, P, None, 0), b"bad top_p"),
        ((None, 0, P, 8, 1, 8, P, 1.0, 0, 10.0, P, None, 0), b"bad top_p"),                      # the reference's default
        ((None, 0, P, 8, 1, 8, P, 1.0, 0, nan, P, None, 0), b"bad top_p"),
        ((None, 0, P, 8, 1, 8, P, 1.0, 0, -0.5, P, None, 0), b"bad top_p"),
        ((None, 7, P, 8, 1, 8, P, 1.0, 0, 1.0, P, None, 0), b"bad dtype"),
        ((None, 2 if not half else 1, P, 8, 1, 8, P, 1.0, 0, 1.0, P, None, 0), b"bad dtype"),    # the other build's 16-bit type
        ((None, 7, P, 8, 0, 8, P, 1.0, 0, 1.0, P, None, 0), b"bad dtype"),                       # ... also with nothing to do
    ]
    for args, msg in bad:
        rc = l.setok_sample_rows(*args)
        assert rc == -1 and msg in l.setok_last_error(), (args, l.setok_last_error())
    # nothing to do is not an error (and launches nothing); probs without rows needs no stride
    for dt in (0, 2 if half else 1):
        assert l.setok_sample_rows(None, dt, P, 8, 0, 8, P, 1.0, 0, 1.0, P, None, 0) == 0
        assert l.setok_sample_rows(None, dt, P, 8, 0, 8, P, 0.1, 50, 0.9, P, P, 8) == 0


def test_sampler_validates_like_the_c_call(lib):
    from setok_amd.generation import Sampler
    s = Sampler()
    assert (s.temperature, s.top_k, s.top_p, s.generator, s.u) == (1.0, 0, 1.0, None, None)
    s = Sampler(temperature=0.8, top_k=5, top_p=0.9, u=torch.zeros(4, 2))
    assert (s.temperature, s.top_k, s.top_p) == (0.8, 5, 0.9) and s.u.shape == (4, 2)
    for kw in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=math.nan), dict(temperature=math.inf), dict(top_k=-1),
               dict(top_k=1.5), dict(top_p=0.0), dict(top_p=-0.1), dict(top_p=1.5), dict(top_p=math.nan), dict(u=torch.zeros(4)),
               dict(u=torch.zeros(4, 2, dtype=torch.float64)), dict(u=torch.zeros(4, 2), generator=torch.Generator())):
        with pytest.raises(ValueError):
            Sampler(**kw)
    with pytest.raises(ValueError, match="not a probability"):
        Sampler(temperature=0.1, top_p=10.0)                          # the reference's defaults (setokim_llama.py:341-356)
    with pytest.raises(ValueError, match="step 4"):
        Sampler(u=torch.zeros(4, 2)).uniforms(4, 2, "cpu")            # more steps than rows of u
    with pytest.raises(ValueError):
        Sampler(u=torch.zeros(4, 2)).uniforms(0, 3, "cpu")            # another batch
    u = torch.rand(4, 2)
    assert torch.equal(Sampler(u=u).uniforms(3, 2, "cpu"), u[3])
    a = Sampler(generator=torch.Generator().manual_seed(5)).uniforms(0, 3, "cpu")
    b = Sampler(generator=torch.Generator().manual_seed(5)).uniforms(0, 3, "cpu")
    assert a.dtype == torch.float32 and a.shape == (3,) and torch.equal(a, b)


def test_generate_and_ops_carry_the_surface(lib):
    from setok_amd import llama, ops
    sig = inspect.signature(llama.SetokimLlamaPrefill.generate)
    assert sig.parameters["sampler"].default is None and sig.parameters["do_sample"].default is False
    assert "sampler=" in llama.SetokimLlamaPrefill.generate.__doc__
    sig = inspect.signature(ops.sample_rows)
    assert [(k, p.default) for k, p in sig.parameters.items()][2:] == [("temperature", 1.0), ("top_k", 0), ("top_p", 1.0), ("out", None), ("probs", None)]


def test_the_case_list_covers_the_grid():
    cs = S.CASES.values()
    assert {c["V"] for c in cs} == {1, 7, 257, 32000, 128256} and {c["rows"] for c in cs} == {1, 3, 33}
    assert {c["dt"] for c in cs} == {"fp32", "bf16", "fp16"} and {c["T"] for c in cs} == {0.1, 1.0, 2.0}
    assert {c["k"] for c in cs if c["k"] <= c["V"]} == {0, 1, 2, 50} and any(c["k"] == c["V"] + 5 for c in cs)
    for V in (257, 32000, 128256):                                    # every filter at every size that has room for it
        kinds = {(0 < c["k"] < V, c["p"]) for c in cs if c["V"] == V}
        assert kinds == {(False, False), (True, False), (False, True), (True, True)}, V
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "sample.npz")) <= golden_io.LIMIT


@pytest.mark.parametrize("name", list(S.CASES))
def test_fixture_shapes_kept_sets_and_margins(golden, name):
    """The fixture is HF's; sample_cases' fp64 rule reproduces it: the same top_p and u, the same kept set, the same probabilities and tokens; and
    every constructed u lies at least 5e-4 inside the CDF interval of its token, every top_p at least 1e-3 from the nearest "mass above"."""
    c, z = S.CASES[name], golden
    rows, V = c["rows"], c["V"]
    built = S.build(name)
    x = S.logits(name)
    assert x.shape == (rows, V) and x.dtype == S.DTYPES[c["dt"]]
    top_p, u, tokens = z[name + ":top_p"], z[name + ":u"], z[name + ":tokens"]
    assert top_p.shape == u.shape == tokens.shape == (rows,) and top_p.dtype == u.dtype == np.float32 and z[name + ":hf_err"].shape == (2,)
    assert np.array_equal(top_p, np.array([b["top_p"] for b in built], np.float32)) and np.array_equal(u, np.array([b["u"] for b in built], np.float32))
    assert np.array_equal(tokens, [b["token"] for b in built]) and np.array_equal(z[name + ":kept_count"], [int(b["keep"].sum()) for b in built])
    assert (top_p < 1.0).all() if c["p"] else (top_p == 1.0).all()
    for r, b in enumerate(built):
        lo, hi = S.intervals(b["p"])
        t = int(tokens[r])
        assert b["keep"][t] and b["p"][t] > 1e-3 and lo[t] + 5e-4 <= float(u[r]) <= hi[t] - 5e-4, (r, lo[t], float(u[r]), hi[t])
        s = S.scores(x[r], c["T"])
        if c["p"]:
            above = S.mass_above(s, S.topk_keep(s, c["k"]))
            assert np.abs(above[np.isfinite(s)] - float(top_p[r])).min() >= 1e-3 - 1e-7, r
        if c["ninf"]:
            assert not np.isfinite(s).all() and b["p"][~np.isfinite(s)].max() == 0.0
        mt, mp = S.fixed_point_draw(x[r], c["T"], c["k"], float(top_p[r]), float(u[r]))      # the kernel's arithmetic, modelled on the CPU
        assert mt == t and np.abs(mp - b["p"]).max() < 2e-6, (r, mt, t)
        if S.filtered(c):
            sel = z[name + ":kept_row"] == r
            assert np.array_equal(z[name + ":kept_idx"][sel], np.nonzero(b["keep"])[0])
            assert np.abs(z[name + ":kept_p"][sel] - b["p"][b["keep"]]).max() < 1e-12
        else:
            idx = z[name + ":top_idx"][r]
            idx = idx[idx >= 0]
            assert np.abs(z[name + ":top_p64"][r][:idx.size] - b["p"][idx]).max() < 1e-12
            assert np.array_equal(np.sort(b["p"])[::-1][:idx.size], b["p"][idx])
