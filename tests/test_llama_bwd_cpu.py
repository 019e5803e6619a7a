"""The backward pass through the frozen Llama, without a GPU: the five new C-ABI entries are declared, exported by both builds and mirrored by
the ctypes table; they validate their arguments on the host before any launch; and the committed fixture tests/golden/llama_bwd.npz
(HuggingFace LlamaForCausalLM under torch autograd, tests/golden/make_golden_llama_bwd.py) is pinned to the oracle's restatement, so a
regenerated fixture cannot drift unnoticed."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import golden_io
import llama_bwd_cases as C
import setok_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"setok_lm_loss_bwd": 14, "setok_rmsnorm_bwd": 10, "setok_rope_bwd_gqa": 9, "setok_swiglu_pairs_bwd": 7,
       "setok_attention_causal_bwd_gqa": 14, "setok_attention_causal_bwd": 13}


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    from setok_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH) or not os.path.isfile(_lib.LIB_PATH_F16):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_new_entries_are_declared_exported_and_in_the_ctypes_table(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "setok_hip.h")).read(), flags=re.S)
    decls = {n: [a for a in args.split(",") if a.strip()] for n, args in re.findall(r"\bint\s+(setok_\w+)\s*\(([^;]*)\)\s*;", text, flags=re.S)}
    for name, arity in NEW.items():
        assert name in decls and len(decls[name]) == arity, name
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name]) == arity, name
        for path in (lib.LIB_PATH, lib.LIB_PATH_F16):
            assert hasattr(ctypes.CDLL(path), name), f"{name} not exported by {os.path.basename(path)}"
    assert lib.load().setok_abi_version() == 9                     # additive: the ABI version stays


@pytest.mark.parametrize("half", [False, True])
def test_null_operands_and_bad_shapes_are_refused_on_the_host(lib, half):
    l = lib.load(half)
    P = 64                                                            # a non-null "pointer": validation fails before anything is dereferenced or launched
    bad = [
        ("setok_lm_loss_bwd", (None, 0, None, 8, P, None, 1, 2, 8, -100, P, None, P, 8), b"null operand"),
        ("setok_lm_loss_bwd", (None, 0, P, 8, P, None, 1, 2, 8, -100, P, None, None, 8), b"null operand"),
        ("setok_lm_loss_bwd", (None, 0, P, 4, P, None, 1, 2, 8, -100, P, None, P, 8), b"bad shape"),          # ld < V
        ("setok_lm_loss_bwd", (None, 0, P, 8, P, None, 1, 2, 8, -100, P, None, P, 7), b"bad shape"),          # ldd < V
        ("setok_rmsnorm_bwd", (None, 0, P, P, None, None, P, 1, 64, 1e-5), b"null operand"),
        ("setok_rmsnorm_bwd", (None, 0, P, P, P, None, P, 1, 12, 1e-5), b"multiple of 8"),
        ("setok_rope_bwd_gqa", (None, 0, None, P, 1, 4, 2, 16, 10000.0), b"null operand"),
        ("setok_rope_bwd_gqa", (None, 0, P, P, 1, 4, 3, 16, 10000.0), b"bad shape"),                         # H % Hkv
        ("setok_rope_bwd_gqa", (None, 0, P, P, 1, 4, 2, 15, 10000.0), b"bad shape"),                         # odd head dim
        ("setok_swiglu_pairs_bwd", (None, 0, P, None, P, 1, 8), b"null operand"),
        ("setok_swiglu_pairs_bwd", (None, 0, P, P, P, 1, 12), b"multiple of 8"),
        ("setok_attention_causal_bwd_gqa", (None, 0, P, None, P, P, P, 1, 4, 4, 2, 16, 0.25, None), b"null operand"),   # no workspace
        ("setok_attention_causal_bwd_gqa", (None, 0, P, None, P, None, P, 1, 4, 4, 2, 16, 0.25, P), b"null operand"),
        ("setok_attention_causal_bwd_gqa", (None, 0, P, None, P, P, P, 1, 4, 4, 3, 16, 0.25, P), b"bad shape"),
        ("setok_attention_causal_bwd_gqa", (None, 0, P, None, P, P, P, 1, 0, 4, 2, 16, 0.25, P), b"bad shape"),
        ("setok_attention_causal_bwd_gqa", (None, 0, P, None, P, P, P, 1, 4, 4, 2, 1024, 0.25, P), b"too large"),
        ("setok_attention_causal_bwd_gqa", (None, 7, P, None, P, P, P, 1, 4, 4, 2, 16, 0.25, P), b"bad dtype"),
        ("setok_attention_causal_bwd", (None, 0, None, None, P, P, P, 1, 4, 4, 16, 0.25, P), b"null operand"),
    ]
    for name, args, msg in bad:
        rc = getattr(l, name)(*args)
        assert rc == -1 and msg in l.setok_last_error(), (name, args, l.setok_last_error())
    other = 1 if half else 2                                          # the other build's 16-bit type is refused, never read as something else
    assert l.setok_rmsnorm_bwd(None, other, P, P, P, None, P, 1, 64, 1e-5) == -1
    assert l.setok_attention_causal_bwd(None, other, P, None, P, P, P, 1, 4, 4, 16, 0.25, P) == -1


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _rel(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("name", list(C.LLAMA_CASES))
def test_fixture_is_the_oracles_gradient_and_zero_at_padded_rows(golden_dir, name):
    """d loss / d inputs_embeds and d sum(hidden * G) / d inputs_embeds of tests/golden/llama_bwd.npz (HF's autograd) against the oracle's
    llama_forward + lm_loss under torch autograd on the regenerated inputs: <= 1e-6 max-rel at the attended rows; exact zeros at padded rows,
    in the fp32 and in the 16-bit yardstick gradients."""
    z = golden_io.load(os.path.join(golden_dir, "llama_bwd.npz"))
    kw, lc, seed, x, am, pos, labels, G = C.case_inputs(name)
    assert [int(v) for v in z[name + ":spec"]] == [seed, x.shape[0], x.shape[1], 1 if C.LLAMA_CASES[name][4] == "left" else 0]
    assert C.first_attended_label_is_ignored(labels, am)
    sd = O.init_llama_weights(lc, seed=seed)
    with torch.enable_grad():
        xe = x.clone().requires_grad_(True)
        h, lg = O.llama_forward(sd, lc, xe, am, pos)
        loss = O.lm_loss(lg, labels, am)
        (g_loss,) = torch.autograd.grad(loss, xe, retain_graph=True)
        (g_hid,) = torch.autograd.grad((h * G).sum(), xe)
    assert abs(float(loss.detach()) - float(z[name + ":loss"][0])) <= 1e-6 * abs(float(loss.detach()))
    v = am.bool()
    assert _rel(g_loss[v], _t(z[name + ":dx_loss"])[v]) <= 1e-6
    assert _rel(g_hid[v], _t(z[name + ":dx_hidden"])[v]) <= 1e-6
    keys = [k for k in z.files if k.startswith(name + ":dx_")]
    assert len(keys) == (6 if name in C.DH128 else 2)                # fp32 (+ HF's own bf16 and fp16 runs for the head-dim-128 cases)
    for k in keys:
        g = _t(z[k])
        assert g.shape == x.shape and float(g[v].abs().max()) > 0
        if (~v).any():
            assert float(g[~v].abs().max()) == 0.0, k


def test_stage2_llm_fixture_loads_and_is_mostly_nonzero(golden_dir):
    z = golden_io.load(os.path.join(golden_dir, "stage2_llm.npz"))
    for name in C.STAGE2_LLM_CASES:
        c = C.stage2_llm_inputs(name)
        dt = _t(z[name + ":dtokens"])
        assert dt.shape == (sum(t.shape[0] for t in c["toks"]), c["Dt"])
        assert 2 * int((dt.abs().sum(1) != 0).sum()) > dt.shape[0]
        assert (name + ":dembed" in z) == c["train_embed"]
        assert _t(z[name + ":embeds"]).shape[1] == c["kw"]["max_length"]      # the batch was truncated
