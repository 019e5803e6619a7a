"""LoRA without a device: the skinny GEMM's entry points are declared, exported and mirrored; setok_linear_skinny refuses what it cannot compute on
the host, before any launch, with the argument named; add_lora_ builds, names, initialises and freezes what it says and refuses by name; the
adapter state dict round-trips in both spellings; the inference entry points refuse unmerged adapters before any device call."""
import math
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

P = 4096        # stands in for a device pointer: the calls below are refused before anything is launched or dereferenced
TINY = dict(hidden_size=64, intermediate_size=176, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, vocab_size=100)
NEW = ("setok_linear_skinny_workspace", "setok_linear_skinny")


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    from setok_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH) or not os.path.isfile(_lib.LIB_PATH_F16):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


@pytest.fixture()
def tiny(lib):
    from setok_amd.llama import SetokimLlamaPrefill
    torch.manual_seed(0)
    return SetokimLlamaPrefill(dict(TINY))


def test_the_two_symbols_are_declared_exported_by_both_builds_and_mirrored(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "setok_hip.h")).read(), flags=re.S)
    for name in NEW:
        decl = re.search(r"\b(?:int64_t|int)\s+" + name + r"\s*\(([^;]*)\)\s*;", text, flags=re.S)
        assert decl, f"{name} is not declared in include/setok_hip.h"
        assert len(decl.group(1).split(",")) == len(lib.SIGNATURES[name])
        for half in (False, True):
            assert hasattr(lib.load(half), name)
    assert lib.RESTYPES["setok_linear_skinny_workspace"] is lib._i64
    assert re.search(r"#define\s+SETOK_SKINNY_MAX_N\s+256", text) and re.search(r"#define\s+SETOK_SKINNY_KSLICE\s+\d+", text)
    assert lib.load().setok_abi_version() == 9 and lib.load(half=True).setok_abi_version() == 9      # additions: the ABI version stays


def test_the_workspace_rule_and_the_slice_read_off_it(lib):
    from setok_amd import ops
    ks = ops.skinny_kslice()
    declared = int(re.search(r"#define\s+SETOK_SKINNY_KSLICE\s+(\d+)", open(os.path.join(ROOT, "include", "setok_hip.h")).read()).group(1))
    assert ks == declared == ops.skinny_kslice(half=True) and ks % 64 == 0
    for half in (False, True):
        l = lib.load(half)
        assert l.setok_linear_skinny_workspace(200, 128, ks) == 200 * 128
        assert l.setok_linear_skinny_workspace(200, 128, ks + 64) == 2 * 200 * 128
        assert l.setok_linear_skinny_workspace(17664, 256, 11008) == math.ceil(11008 / ks) * 17664 * 256      # past 2^31 bytes: 64-bit
        assert l.setok_linear_skinny_workspace(0, 128, 512) == 0


def _args(dtype, out_dtype=None, A=P, W=P, C=P, ws=P, M=4, N=64, K=64, lda=64, ldw=64, ldc=64, alpha=1.0, ws_floats=None, lib=None):
    # setok_linear_skinny(stream, dtype, out_dtype, A, lda, W, ldw, C, ldc, M, N, K, alpha, ws, ws_floats)
    need = lib.setok_linear_skinny_workspace(M, N, K)
    return (None, dtype, dtype if out_dtype is None else out_dtype, A, lda, W, ldw, C, ldc, M, N, K, alpha, ws, need if ws_floats is None else ws_floats)


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("kw,fp32,names", [
    (dict(N=272, ldc=272), False, b"N=272"),                          # wider than SETOK_SKINNY_MAX_N
    (dict(N=272, ldc=272), True, b"N=272"),
    (dict(N=24, ldc=24), False, b"N=24"),                             # N % 16
    (dict(N=24, ldc=24), True, b"N=24"),
    (dict(K=96, lda=96, ldw=96), False, b"K=96"),                     # 16-bit: K % 64
    (dict(K=24, lda=24, ldw=24), True, b"K=24"),                      # fp32: K % 16
    (dict(lda=56), False, b"lda=56"),                                 # lda < K
    (dict(lda=48), True, b"lda=48"),
    (dict(ldw=48), False, b"ldw=48"),
    (dict(ldc=48), False, b"ldc=48"),
    (dict(lda=68), False, b"lda=68"),                                 # 16-byte pieces
    (dict(A=None), False, b"null operand"),
    (dict(W=None), True, b"null operand"),
    (dict(C=None), False, b"null operand"),
    (dict(M=-1), False, b"M=-1"),
])
def test_linear_skinny_refuses_on_the_host_with_the_argument_named(lib, half, kw, fp32, names):
    l = lib.load(half)
    dt = 0 if fp32 else (2 if half else 1)
    assert l.setok_linear_skinny(*_args(dt, lib=l, **kw)) == -1
    assert names in l.setok_last_error(), l.setok_last_error()


@pytest.mark.parametrize("half", [False, True])
def test_linear_skinny_refuses_a_short_workspace_a_bad_output_type_and_the_other_builds_type(lib, half):
    l = lib.load(half)
    dt = 2 if half else 1
    for d in (0, dt):
        K = 2048
        need = l.setok_linear_skinny_workspace(4, 64, K)
        assert need > 4 * 64                                                                  # several slices
        assert l.setok_linear_skinny(*_args(d, lib=l, K=K, lda=K, ldw=K, ws_floats=need - 1)) == -1           # one float short
        assert b"workspace" in l.setok_last_error() and str(need).encode() in l.setok_last_error(), l.setok_last_error()
        assert l.setok_linear_skinny(*_args(d, lib=l, ws=None)) == -1 and b"workspace" in l.setok_last_error()
    assert l.setok_linear_skinny(*_args(0, out_dtype=dt, lib=l)) == -1 and b"out_dtype" in l.setok_last_error()      # fp32 inputs, 16-bit output
    assert l.setok_linear_skinny(*_args(1 if half else 2, lib=l)) == -1 and b"dtype" in l.setok_last_error()


# ---- add_lora_ --------------------------------------------------------------------------------------------------------------------------
def test_add_lora_names_shapes_init_and_what_it_freezes(tiny):
    from setok_amd.lora import ALL_SEVEN
    m = tiny
    assert m.model.lora is None and all(p.requires_grad for p in m.parameters())
    base = {k: v.clone() for k, v in m.state_dict().items()}
    assert m.add_lora_(16, 32, lora_dropout=0.05) is m
    ad = m.model.lora
    assert ad.r == 16 and ad.scaling == 2.0 and ad.lora_dropout == 0.05 and ad.targets == ALL_SEVEN
    D, Fd, kv = 64, 176, 32
    shapes = {"q_proj": (D, D), "k_proj": (kv, D), "v_proj": (kv, D), "o_proj": (D, D), "gate_proj": (Fd, D), "up_proj": (Fd, D), "down_proj": (D, Fd)}
    names = {n for n, _ in m.named_parameters() if "lora" in n}
    assert names == {f"model.lora.layers.{i}.{t}.lora_{ab}" for i in range(2) for t in ALL_SEVEN for ab in "AB"}
    assert not any(n.startswith("model.layers.") and "lora" in n for n in names)             # outside self.layers
    for i in range(2):
        for t, (o, ii) in shapes.items():
            p = ad.layers[i][t]
            assert tuple(p.lora_A.shape) == (16, ii) and tuple(p.lora_B.shape) == (o, 16) and p.lora_A.dtype == p.lora_B.dtype == torch.float32
            assert float(p.lora_B.detach().abs().max()) == 0.0                                      # peft: B = 0 ...
            bound = 1.0 / math.sqrt(ii)                                                       # ... A Kaiming-uniform with a = sqrt(5): U(-1 / sqrt(in), 1 / sqrt(in))
            assert float(p.lora_A.detach().abs().max()) <= bound and float(p.lora_A.detach().abs().max()) > 0.9 * bound
            assert abs(float(p.lora_A.detach().std()) - bound / math.sqrt(3)) < 0.1 * bound and abs(float(p.lora_A.detach().mean())) < 0.1 * bound
            assert p.lora_A.requires_grad and p.lora_B.requires_grad
    trainable = {n for n, p in m.named_parameters() if p.requires_grad}
    assert trainable == names | {"model.embed_tokens.weight"}                                 # layers.*, norm and lm_head frozen; embed_tokens is not part of the stack
    assert not m.model.stack_requires_grad()
    assert all(torch.equal(m.state_dict()[k], v) for k, v in base.items())                    # no base weight touched
    sub = type(m)(dict(TINY)).model.add_lora_(16, 16, target_modules=("v_proj", "q_proj"))
    assert sub.lora.targets == ("q_proj", "v_proj") and sub.lora.scaling == 1.0 and len(list(sub.lora.parameters())) == 8
    assert not sub.stack_requires_grad()


def test_add_lora_refuses_by_name(tiny, lib):
    from setok_amd.llama import SetokimLlamaPrefill
    with pytest.raises(ValueError, match="r=8 .*multiple of 16"):
        tiny.add_lora_(8, 16)
    with pytest.raises(ValueError, match="r=24 .*multiple of 16"):
        tiny.add_lora_(24, 16)
    with pytest.raises(ValueError, match="r=16 .*multiple of 64"):                              # the 16-bit types: the GEMM's K granule is 64
        SetokimLlamaPrefill(dict(TINY)).to(torch.bfloat16).add_lora_(16, 32)
    with pytest.raises(ValueError, match="r=0 "):
        tiny.add_lora_(0, 16)
    with pytest.raises(ValueError, match=r"unknown target_modules \['lm_head'\]"):
        tiny.add_lora_(16, 32, target_modules=("q_proj", "lm_head"))
    assert tiny.model.lora is None and tiny.model.stack_requires_grad()                        # a refused request changes nothing
    tiny.add_lora_(16, 32)
    with pytest.raises(NotImplementedError, match="already attached"):
        tiny.add_lora_(16, 32)
    fp8 = SetokimLlamaPrefill(dict(TINY))
    fp8.model._quant = dict(fmt=sys.modules["setok_amd.llama"]._FP8)                           # (what quantize_fp8_ leaves behind; it needs a device)
    with pytest.raises(NotImplementedError, match="fp8 storage"):
        fp8.add_lora_(16, 32)
    for call in (lambda: SetokimLlamaPrefill(dict(TINY)).lora_state_dict(), lambda: SetokimLlamaPrefill(dict(TINY)).merge_lora_(),
                 lambda: SetokimLlamaPrefill(dict(TINY)).load_lora_state_dict({})):
        with pytest.raises(ValueError, match="no adapters are attached"):
            call()


def test_the_state_dict_keys_round_trip_in_both_spellings(tiny):
    import lora_cases as LC
    import setok_oracle as O  # noqa: F401  (conftest puts oracle/ on the path)
    from setok_amd.llama import SetokimLlamaPrefill
    lc = O.LlamaConfigLite(**TINY)
    tiny.add_lora_(16, 32)
    sd = tiny.lora_state_dict()
    assert len(sd) == 2 * 7 * 2 and "base_model.model.model.layers.1.mlp.down_proj.lora_B.weight" in sd
    assert "base_model.model.model.layers.0.self_attn.q_proj.lora_A.weight" in sd and all(".default." not in k for k in sd)
    assert tuple(sd["base_model.model.model.layers.0.self_attn.k_proj.lora_B.weight"].shape) == (32, 16)
    ad = LC.adapters(lc, 16, seed=3)
    assert set(LC.peft_keys(ad)) == set(sd)
    tiny.load_lora_state_dict(LC.peft_keys(ad))
    got = tiny.lora_state_dict()
    assert all(torch.equal(got[k], v) for k, v in LC.peft_keys(ad).items())
    other = SetokimLlamaPrefill(dict(TINY)).add_lora_(16, 32)
    other.load_lora_state_dict({k.replace(".weight", ".default.weight"): v for k, v in got.items()})       # the in-memory PeftModel spelling
    assert all(torch.equal(other.lora_state_dict()[k], v) for k, v in got.items())
    assert torch.equal(other.model.lora.layers[1]["up_proj"].lora_B, ad["1.up_proj.lora_B"])
    with pytest.raises(KeyError, match="unexpected key"):
        other.load_lora_state_dict(dict(got, **{"base_model.model.lm_head.lora_A.weight": torch.zeros(1)}))
    with pytest.raises(KeyError, match="missing keys"):
        other.load_lora_state_dict({k: v for k, v in got.items() if "layers.0" in k})
    with pytest.raises(ValueError, match="shape"):
        other.load_lora_state_dict({k: v[:8] for k, v in got.items()})
    assert all(k.startswith("model.lora.") for k in other.state_dict() if "lora" in k) and any("lora" in k for k in other.state_dict())


def test_inference_entry_points_refuse_unmerged_adapters_before_any_device_call(tiny):
    tiny.add_lora_(16, 32)
    x = torch.zeros(1, 3, 64)                                                                  # host tensors: a device call would fail differently
    with pytest.raises(NotImplementedError, match=r"generate.*merge_lora_\(\)"):
        tiny.generate(inputs_embeds=x, max_new_tokens=2)
    with pytest.raises(NotImplementedError, match=r"prefill.*merge_lora_\(\)"):
        tiny.model.prefill(x, cache=None)
    with pytest.raises(NotImplementedError, match=r"decode_step.*merge_lora_\(\)"):
        tiny.model.decode_step(x[:, 0], cache=None)
    with pytest.raises(NotImplementedError, match=r"extend.*merge_lora_\(\)"):
        tiny.model.extend(x, cache=None)
    for q in (tiny.quantize_fp8_, tiny.model.quantize_fp8_):
        with pytest.raises(NotImplementedError, match=r"quantize_fp8_.*merge_lora_\(\)"):
            q()
    assert tiny.weight_format == "native"
