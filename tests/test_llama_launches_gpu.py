"""The library calls behind `LlamaModel`'s entry points, by symbol name and in order: `_forward` / `prefill`, `decode_step` and `extend` run the
stack through one layer loop, and what can go wrong there is an extra, a missing or a reordered call - which no parity test sees when the call
happens to be harmless.  `setok_amd._lib.call` is wrapped by a recorder that notes the symbol and calls through; the recorded list must equal the
literal one below, which is `LAYER[name]` once per decoder layer followed by `TAIL`.  The literals were recorded on the commit BEFORE the three loops were
folded into one (the same recorder over the three written-out loops), so they pin the sequence the refactor had to keep.  The two smallest cases of
tests/llama_bwd_cases.py are enough: the loop body is shape-blind.  `pytest -m gpu`."""
import pytest
import torch

import llama_bwd_cases as C
import setok_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from setok_amd import _lib
    from setok_amd.generation import KVCache
    from setok_amd.llama import SetokimLlamaPrefill

DEV = "cuda"
CASES = {"tiny": ("tiny_left", torch.float32), "dh128": ("dh128_left", torch.bfloat16)}
_MODELS = {}

# name: (case, weights, kv cache or None, entry point, rows: B of a decode step on a hand-filled cache, Tn of an extend)
SCENARIOS = {}
for _c in CASES:
    SCENARIOS[f"{_c}-forward"] = (_c, "native", None, "prefill", 0)
    for _kv in ("native", "fp8") + (("mxfp4",) if _c == "dh128" else ()):      # (an mxfp4 cache needs a head dim that is a multiple of 32)
        SCENARIOS[f"{_c}-prefill-{_kv}kv"] = (_c, "native", _kv, "prefill", 0)
        SCENARIOS[f"{_c}-decode-{_kv}kv"] = (_c, "native", _kv, "decode", 0)
    SCENARIOS[f"{_c}-extend3-nativekv"] = (_c, "native", "native", "extend", 3)
    for _w in ("fp8",) + (("mxfp4",) if _c == "dh128" else ()):                # (mxfp4 weights need in_features on the K granule: not 176)
        SCENARIOS[f"{_c}-{_w}w-decode"] = (_c, _w, "native", "decode", 0)      # B = 3 and 2: the weight-streaming GEMM
        SCENARIOS[f"{_c}-{_w}w-decode-B65"] = (_c, _w, "native", "decode", 65)  # above max_m = 64: dequantise, then `linear`
SCENARIOS["dh128-extend3-mxfp4kv"] = ("dh128", "native", "mxfp4", "extend", 3)
SCENARIOS["dh128-fp8w-extend-M16"] = ("dh128", "fp8", "native", "extend", 8)     # B * Tn = 16 and 80: the two shapes of test_extend_gpu.py
SCENARIOS["dh128-fp8w-extend-M80"] = ("dh128", "fp8", "native", "extend", 40)

# One decoder layer's calls per scenario, as the commit before the single layer loop made them; an entry point's list is this once per layer + TAIL.
LAYER = {
    "tiny-forward": ["setok_rmsnorm", "setok_linear", "setok_rope_gqa", "setok_attention_causal_gqa", "setok_linear", "setok_rmsnorm", "setok_linear", "setok_swiglu_pairs", "setok_linear"],
    "tiny-prefill-nativekv": ["setok_rmsnorm", "setok_linear", "setok_rope_gqa", "setok_kv_append", "setok_attention_causal_gqa", "setok_linear", "setok_rmsnorm", "setok_linear", "setok_swiglu_pairs", "setok_linear"],
    "tiny-decode-nativekv": ["setok_rmsnorm", "setok_linear", "setok_rope_gqa", "setok_kv_append", "setok_attention_decode_gqa", "setok_linear", "setok_rmsnorm", "setok_linear", "setok_swiglu_pairs", "setok_linear"],
    "tiny-prefill-fp8kv": ["setok_rmsnorm", "setok_linear", "setok_rope_gqa", "setok_kv_append_fp8", "setok_attention_causal_gqa", "setok_linear", "setok_rmsnorm", "setok_linear", "setok_swiglu_pairs", "setok_linear"],
    "tiny-decode-fp8kv": ["setok_rmsnorm", "setok_linear", "setok_rope_gqa", "setok_kv_append_fp8", "setok_attention_decode_gqa_fp8kv", "setok_linear", "setok_rmsnorm", "setok_linear", "setok_swiglu_pairs", "setok_linear"],
    "tiny-extend3-nativekv": ["setok_rmsnorm", "setok_linear", "setok_rope_gqa", "setok_kv_append", "setok_attention_extend_gqa", "setok_linear", "setok_rmsnorm", "setok_linear", "setok_swiglu_pairs", "setok_linear"],
    "tiny-fp8w-decode": ["setok_rmsnorm", "setok_linear_fp8w", "setok_rope_gqa", "setok_kv_append", "setok_attention_decode_gqa", "setok_linear_fp8w", "setok_rmsnorm", "setok_linear_fp8w", "setok_swiglu_pairs", "setok_linear_fp8w"],
    "tiny-fp8w-decode-B65": ["setok_rmsnorm", "setok_dequantize_fp8_rows", "setok_linear", "setok_rope_gqa", "setok_kv_append", "setok_attention_decode_gqa", "setok_dequantize_fp8_rows", "setok_linear", "setok_rmsnorm", "setok_dequantize_fp8_rows", "setok_linear", "setok_swiglu_pairs", "setok_dequantize_fp8_rows", "setok_linear"],
    "dh128-forward": ["setok_rmsnorm", "setok_linear", "setok_rope_gqa", "setok_attention_causal_gqa", "setok_linear", "setok_rmsnorm", "setok_linear", "setok_swiglu_pairs", "setok_linear"],
    "dh128-prefill-nativekv": ["setok_rmsnorm", "setok_linear", "setok_rope_gqa", "setok_kv_append", "setok_attention_causal_gqa", "setok_linear", "setok_rmsnorm", "setok_linear", "setok_swiglu_pairs", "setok_linear"],
    "dh128-decode-nativekv": ["setok_rmsnorm", "setok_linear", "setok_rope_gqa", "setok_kv_append", "setok_attention_decode_gqa", "setok_linear", "setok_rmsnorm", "setok_linear", "setok_swiglu_pairs", "setok_linear"],
    "dh128-prefill-fp8kv": ["setok_rmsnorm", "setok_linear", "setok_rope_gqa", "setok_kv_append_fp8", "setok_attention_causal_gqa", "setok_linear", "setok_rmsnorm", "setok_linear", "setok_swiglu_pairs", "setok_linear"],
    "dh128-decode-fp8kv": ["setok_rmsnorm", "setok_linear", "setok_rope_gqa", "setok_kv_append_fp8", "setok_attention_decode_gqa_fp8kv", "setok_linear", "setok_rmsnorm", "setok_linear", "setok_swiglu_pairs", "setok_linear"],
    "dh128-prefill-mxfp4kv": ["setok_rmsnorm", "setok_linear", "setok_rope_gqa", "setok_kv_append_mxfp4", "setok_attention_causal_gqa", "setok_linear", "setok_rmsnorm", "setok_linear", "setok_swiglu_pairs", "setok_linear"],
    "dh128-decode-mxfp4kv": ["setok_rmsnorm", "setok_linear", "setok_rope_gqa", "setok_kv_append_mxfp4", "setok_attention_decode_gqa_mxfp4kv", "setok_linear", "setok_rmsnorm", "setok_linear", "setok_swiglu_pairs", "setok_linear"],
    "dh128-extend3-nativekv": ["setok_rmsnorm", "setok_linear", "setok_rope_gqa", "setok_kv_append", "setok_attention_extend_gqa", "setok_linear", "setok_rmsnorm", "setok_linear", "setok_swiglu_pairs", "setok_linear"],
    "dh128-fp8w-decode": ["setok_rmsnorm", "setok_linear_fp8w", "setok_rope_gqa", "setok_kv_append", "setok_attention_decode_gqa", "setok_linear_fp8w", "setok_rmsnorm", "setok_linear_fp8w", "setok_swiglu_pairs", "setok_linear_fp8w"],
    "dh128-fp8w-decode-B65": ["setok_rmsnorm", "setok_dequantize_fp8_rows", "setok_linear", "setok_rope_gqa", "setok_kv_append", "setok_attention_decode_gqa", "setok_dequantize_fp8_rows", "setok_linear", "setok_rmsnorm", "setok_dequantize_fp8_rows", "setok_linear", "setok_swiglu_pairs", "setok_dequantize_fp8_rows", "setok_linear"],
    "dh128-mxfp4w-decode": ["setok_rmsnorm", "setok_linear_mxfp4w", "setok_rope_gqa", "setok_kv_append", "setok_attention_decode_gqa", "setok_linear_mxfp4w", "setok_rmsnorm", "setok_linear_mxfp4w", "setok_swiglu_pairs", "setok_linear_mxfp4w"],
    "dh128-mxfp4w-decode-B65": ["setok_rmsnorm", "setok_dequantize_mxfp4_rows", "setok_linear", "setok_rope_gqa", "setok_kv_append", "setok_attention_decode_gqa", "setok_dequantize_mxfp4_rows", "setok_linear", "setok_rmsnorm", "setok_dequantize_mxfp4_rows", "setok_linear", "setok_swiglu_pairs", "setok_dequantize_mxfp4_rows", "setok_linear"],
    "dh128-extend3-mxfp4kv": ["setok_rmsnorm", "setok_linear", "setok_rope_gqa", "setok_kv_append_mxfp4", "setok_attention_extend_gqa_mxfp4kv", "setok_linear", "setok_rmsnorm", "setok_linear", "setok_swiglu_pairs", "setok_linear"],
    "dh128-fp8w-extend-M16": ["setok_rmsnorm", "setok_linear_fp8w", "setok_rope_gqa", "setok_kv_append", "setok_attention_extend_gqa", "setok_linear_fp8w", "setok_rmsnorm", "setok_linear_fp8w", "setok_swiglu_pairs", "setok_linear_fp8w"],
    "dh128-fp8w-extend-M80": ["setok_rmsnorm", "setok_dequantize_fp8_rows", "setok_linear", "setok_rope_gqa", "setok_kv_append", "setok_attention_extend_gqa", "setok_dequantize_fp8_rows", "setok_linear", "setok_rmsnorm", "setok_dequantize_fp8_rows", "setok_linear", "setok_swiglu_pairs", "setok_dequantize_fp8_rows", "setok_linear"],
}
TAIL = ["setok_rmsnorm"]


def _model(case, weights):
    name, dt = CASES[case]
    kw, lc, seed, x, am, pos, _, _ = C.case_inputs(name)
    if (case, weights) not in _MODELS:
        m = SetokimLlamaPrefill(kw)
        m.load_state_dict(O.init_llama_weights(lc, seed=seed), strict=True)
        m = m.to(device=DEV, dtype=dt).eval()
        if weights != "native":
            getattr(m, f"quantize_{weights}_")()
        _MODELS[case, weights] = m
    return _MODELS[case, weights].model, x.to(DEV), am.to(DEV), pos.to(DEV)


def record(monkeypatch, name):
    """The symbols of the scenario's one entry-point call, in order (what precedes it - a prefill that fills the cache - is not recorded)."""
    case, weights, kv, entry, rows = SCENARIOS[name]
    model, x, am, pos = _model(case, weights)
    B, T, D = x.shape
    calls, through = [], _lib.call

    def recorder(sym, *args, **kw):
        calls.append(sym)
        return through(sym, *args, **kw)

    def run(fn):
        with monkeypatch.context() as mp:
            mp.setattr(_lib, "call", recorder)
            fn()

    if entry == "prefill":
        if kv is None:
            run(lambda: model._forward(x, am, pos))
        else:
            cache = KVCache.for_model(model, B, T, kv_format=kv)
            run(lambda: model.prefill(x, am, pos, cache))
    elif entry == "decode" and rows:                                           # more sequences than the case has: a cache filled by hand (zeros, 4 slots)
        cache = KVCache.for_model(model, rows, 8, kv_format=kv)
        cache.key_mask[:, :4], cache.len = 1, 4
        cache.next_pos.fill_(4)
        step = torch.randn(rows, D, generator=torch.Generator().manual_seed(1)).to(device=DEV, dtype=x.dtype)
        run(lambda: model.decode_step(step, cache))
    elif entry == "decode":
        cache = KVCache.for_model(model, B, T + 1, kv_format=kv)
        h = model.prefill(x, am, pos, cache)
        run(lambda: model.decode_step(h[:, -1].contiguous(), cache))
    else:                                                                      # the last `rows` columns extend a cache that holds the others
        cache = KVCache.for_model(model, B, T, kv_format=kv)
        model.prefill(x[:, :T - rows], am[:, :T - rows], pos[:, :T - rows], cache)
        run(lambda: model.extend(x[:, T - rows:], cache, am[:, T - rows:]))
    torch.cuda.synchronize()
    return calls


def test_the_scenarios_cover_what_the_quantised_paths_branch_on():
    from setok_amd import ops
    assert ops.FP8W_MAX_M == ops.MXFP4W_MAX_M == 64                              # B = 2 and 3 stream, B = 65 dequantises; B * Tn = 16 streams, 80 dequantises


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_an_entry_point_makes_exactly_the_recorded_calls(monkeypatch, name):
    layer = LAYER[name]
    got = record(monkeypatch, name)
    print(name, got)
    body, n = got[:-len(TAIL)], len(got[:-len(TAIL)]) // 2
    assert [body[:n], body[n:]] == [body[:n]] * 2, f"{name}: layer 1 does not make layer 0's calls"
    assert got == layer * 2 + TAIL
