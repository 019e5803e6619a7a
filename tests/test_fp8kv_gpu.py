"""The fp8 KV cache on a real MI355X (include/setok_hip.h, "FP8 KV cache"): setok_kv_append_fp8 against the CPU oracle of the storage contract
(tests/fp8_cases.py) bit for bit, setok_attention_decode_gqa_fp8kv against the fp64 attention over the dequantised cache K', V', and
`prefill` / `decode_step` / `generate(kv_cache="fp8")` against a FAKE-QUANTISED NATIVE ARM: the unchanged native path whose appended cache
slots are round-tripped through the oracle's quantiser on the CPU.  K', V' are exact in every element type, so no test here carries a tolerance
for quantisation error.  `pytest -m gpu`."""
import functools

import pytest
import torch

import fp8_cases as F
import llama_bwd_cases as C
import parity
import setok_oracle as O
from test_generate_gpu import DEV, DTYPES, _decode_ref, _expected_with_eos, _log, _model, _rand, _rel, _tol

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from setok_amd import _lib, ops
    from setok_amd.generation import KVCache
    from setok_amd.llama import SetokimLlamaPrefill

CHUNK = 256                                        # SETOK_DECODE_CHUNK_FP8KV
LENS = (1, 31, 32, 33, CHUNK - 1, CHUNK, CHUNK + 1, 1000, 2049, 127, 128, 129)
NEW = 8
MODEL_CASES = ("tiny_left", "gqa_tiny_left", "dh128", "gqa_dh128", "mqa_dh128_left")


# ---- operators ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("Dh", [16, 64, 128, 24])
def test_kv_append_fp8_equals_the_oracle_bit_for_bit(dt, Dh):
    B, T, H, Hkv, cap, pos0 = 2, 3, 4, 2, 9, 2
    rows = F.quantizer_matrix(B * T * 2 * Hkv, Dh, dt)                 # zeros, both clamps, amax = 448 * 2^-6 and one ulp above, ties, subnormals, -0
    rows[5, 1], rows[5, 3], rows[5, Dh - 1] = float("nan"), float("inf"), float("-inf")
    qkv = _rand(B * T, H + 2 * Hkv, Dh, seed=1).to(dt)
    qkv[:, H:] = rows.reshape(B * T, 2 * Hkv, Dh)                      # row (b, t, j): j < Hkv the k head j, else the v head j - Hkv
    g = torch.Generator().manual_seed(2)
    q0 = [torch.randint(0, 256, (B, Hkv, cap, Dh), generator=g, dtype=torch.uint8).to(DEV) for _ in range(2)]
    e0 = [torch.randint(-128, 128, (B, Hkv, cap), generator=g, dtype=torch.int8).to(DEV) for _ in range(2)]
    k_q, v_q, k_e, v_e = q0[0].clone(), q0[1].clone(), e0[0].clone(), e0[1].clone()
    ops.kv_append_fp8(qkv.reshape(B * T, -1).to(DEV), k_q, k_e, v_q, v_e, T, H, pos0)
    wq, we = F.quantize_rows(rows)
    wq, we = wq.reshape(B, T, 2 * Hkv, Dh), we.reshape(B, T, 2 * Hkv)
    assert int((wq == F.NAN_CODE).sum()) == 3 and we.min() == F.E_MIN and we.max() == F.E_MAX
    assert torch.equal(k_q[:, :, pos0:pos0 + T].cpu(), wq[:, :, :Hkv].transpose(1, 2))
    assert torch.equal(v_q[:, :, pos0:pos0 + T].cpu(), wq[:, :, Hkv:].transpose(1, 2))
    assert torch.equal(k_e[:, :, pos0:pos0 + T].cpu(), we[:, :, :Hkv].transpose(1, 2))
    assert torch.equal(v_e[:, :, pos0:pos0 + T].cpu(), we[:, :, Hkv:].transpose(1, 2))
    keep = torch.ones(cap, dtype=torch.bool, device=DEV)
    keep[pos0:pos0 + T] = False                                        # every other slot: codes and exponents unchanged
    assert torch.equal(k_q[:, :, keep], q0[0][:, :, keep]) and torch.equal(v_q[:, :, keep], q0[1][:, :, keep])
    assert torch.equal(k_e[:, :, keep], e0[0][:, :, keep]) and torch.equal(v_e[:, :, keep], e0[1][:, :, keep])


@functools.lru_cache(maxsize=None)
def _cache_rows(B, Hkv, cap, Dh, seed):
    """(k_q, k_e, v_q, v_e) of a seeded cache: Gaussian rows with per-row scales over five octaves (the exponents differ between rows), quantised
    by the CPU oracle.  Shared between the element types and head counts of a test, never modified (callers clone)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(2):
        x = torch.randn(B * Hkv * cap, Dh, generator=g) * 2.0 ** torch.randint(-2, 3, (B * Hkv * cap, 1), generator=g).float()
        q, e = F.quantize_rows(x)
        out += [q.reshape(B, Hkv, cap, Dh), e.reshape(B, Hkv, cap)]
    return tuple(out)


def _fp8_problem(dt, H, Hkv, Dh, n, cap, seed):
    """_decode_problem of test_generate_gpu.py over an fp8 cache.  Four sequences: all keys, left-padded, right-padded, fully masked.  Dead
    slots (masked, or at / past n) hold the NaN code and exponent bytes 127 and -128 alternately; mask bytes past n are 1."""
    B = 4
    qkv = _rand(B, (H + 2 * Hkv) * Dh, seed=seed).to(dt)
    k_q, k_e, v_q, v_e = [t.clone() for t in _cache_rows(B, Hkv, cap, Dh, seed + 1)]
    mask = torch.zeros(B, cap, dtype=torch.uint8)
    mask[0, :n] = 1
    mask[1, n // 3:n] = 1
    mask[2, :n - n // 4] = 1
    mask[:, n:] = 1
    dead = (mask == 0)[:, None, :].expand(B, Hkv, cap).clone()
    dead[:, :, n:] = True
    bad_e = torch.where(torch.arange(cap) % 2 == 0, 127, -128).to(torch.int8)[None, None].expand(B, Hkv, cap)
    for q, e in ((k_q, k_e), (v_q, v_e)):
        q[dead] = F.NAN_CODE
        e[dead] = bad_e[dead]
    return qkv, k_q, k_e, v_q, v_e, mask


def _dequant(q, e):
    """K' (fp64) of a (B, Hkv, cap, Dh) code tensor and its (B, Hkv, cap) exponents."""
    return F.dequantize_rows(q.reshape(-1, q.shape[-1]), e.reshape(-1)).reshape(q.shape)


def _check_attention(dt, H, Hkv, Dh, n, cap, seed, compare_native):
    qkv, k_q, k_e, v_q, v_e, mask = _fp8_problem(dt, H, Hkv, Dh, n, cap, seed)
    got = ops.attention_decode_fp8kv(qkv.to(DEV), k_q.to(DEV), k_e.to(DEV), v_q.to(DEV), v_e.to(DEV), mask.to(DEV), H, n, Dh ** -0.5).cpu()
    kd, vd = _dequant(k_q, k_e), _dequant(v_q, v_e)                    # (dead slots: NaN, as in _decode_problem)
    ref = _decode_ref(qkv, kd, vd, mask, H, Hkv, Dh, n)
    assert torch.isfinite(got.float()).all(), n
    err, tol = _rel(got, ref), _tol(dt, Dh)
    if compare_native:                                                 # the native kernel over the same K', V' in the element type (exact), for comparison
        nat = ops.attention_decode(qkv.to(DEV), kd.to(dt).to(DEV), vd.to(dt).to(DEV), mask.to(DEV), H, n, Dh ** -0.5).cpu()
        _log(f"fp8kv decode {dt} H={H} Hkv={Hkv} Dh={Dh} len={n}: fp8-cache max-rel, native-on-K'V' max-rel, tol", err, _rel(nat, ref), tol)
    else:
        _log(f"fp8kv decode (generic) {dt} H={H} Hkv={Hkv} Dh={Dh} len={n}: fp8-cache max-rel, tol", err, tol)
    assert err < tol, (n, err, tol)
    assert float(got[3].float().abs().max()) == 0.0, n                 # no key at all -> zeros


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("H,Hkv", [(2, 2), (4, 2), (8, 2), (4, 1), (8, 1)])
@pytest.mark.parametrize("Dh", [16, 64, 128, 32])                      # 1, 4, 8 and 2 lanes per row
def test_attention_decode_fp8kv_against_fp64_on_the_dequantised_cache(dt, H, Hkv, Dh):
    for n in LENS:
        _check_attention(dt, H, Hkv, Dh, n, n + 5, 100 + n, True)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("Dh", [24, 40, 96])
def test_attention_decode_fp8kv_head_dims_outside_the_lane_layouts(dt, Dh):
    for n in (1, CHUNK, CHUNK + 1, 300):
        _check_attention(dt, 4, 2, Dh, n, n + 3, 200 + n, False)


@pytest.mark.parametrize("dt,H,Hkv,Dh", [(torch.bfloat16, 8, 2, 128), (torch.float16, 2, 2, 128), (torch.float32, 4, 2, 16), (torch.bfloat16, 4, 2, 40)])
def test_attention_decode_fp8kv_invariance(dt, H, Hkv, Dh):
    """A sequence's output bits depend on its own q, codes, exponents, mask and len only: not on the batch, not on the capacity, not on the run."""
    n, B = 2 * CHUNK + 37, 5
    cap = n + 3
    g = torch.Generator().manual_seed(9)
    qkv = torch.randn(B, (H + 2 * Hkv) * Dh, generator=g).to(dt).to(DEV)
    k_q, k_e, v_q, v_e = [t.to(DEV) for t in _cache_rows(B, Hkv, cap, Dh, 10)]
    mask = (torch.rand(B, cap, generator=g) > 0.2).to(torch.uint8).to(DEV)
    run = lambda *a: ops.attention_decode_fp8kv(*a, H, n, Dh ** -0.5)
    full = run(qkv, k_q, k_e, v_q, v_e, mask)
    assert torch.equal(full, run(qkv, k_q, k_e, v_q, v_e, mask))                                            # two runs
    b = 2
    alone = run(*[t[b:b + 1].contiguous() for t in (qkv, k_q, k_e, v_q, v_e, mask)])
    assert torch.equal(alone[0], full[b])                                                                   # alone == inside a batch of 5
    def widen(t):                                                      # the slot axis doubled, zeros behind the cache
        dim = 1 if t.dim() == 2 else 2
        w = torch.zeros(t.shape[:dim] + (2 * cap,) + t.shape[dim + 1:], dtype=t.dtype, device=DEV)
        w.narrow(dim, 0, cap).copy_(t)
        return w
    wide = [widen(t) for t in (k_q, k_e, v_q, v_e, mask)]
    assert torch.equal(run(qkv, *wide), full)                                                               # cap == 2 * cap


# ---- model: the fake-quantised native arm ---------------------------------------------------------------------------------------------------
def _fake_quantising_append(real):
    """ops.kv_append followed by a round trip of the appended slots through the CPU oracle: the native cache then holds K', V'."""
    def append(qkv, k_cache, v_cache, T, H, pos0):
        real(qkv, k_cache, v_cache, T, H, pos0)
        for c in (k_cache, v_cache):
            s = c[:, :, pos0:pos0 + T]
            q, e = F.quantize_rows(s.reshape(-1, s.shape[-1]).cpu())
            c[:, :, pos0:pos0 + T] = F.dequantize_rows(q, e).reshape(s.shape).to(device=c.device, dtype=c.dtype)
    return append


def _teacher_forced(m, x, am, pos, tokens, kv_format):
    """test_generate_gpu._teacher_forced with the cache's format as an argument; also returns the cache."""
    n, B = tokens.shape
    T = x.shape[1]
    cache = KVCache.for_model(m.model, B, T + n, kv_format=kv_format)
    hidden = m.model.prefill(x, am, pos, cache)
    last = (am.bool() * torch.arange(T, device=x.device)[None]).max(dim=1).values
    h = hidden[torch.arange(B, device=x.device), last].contiguous()
    w_lm, w_e = m.lm_head.weight.detach().contiguous(), m.model.embed_tokens.weight.detach()
    lgs, hids = [], []
    for j in range(n):
        lgs.append(ops.linear(h, w_lm)); hids.append(h)
        if j + 1 < n:
            h = m.model.decode_step(w_e[tokens[j].to(x.device)], cache)
    assert cache.len == T + n - 1
    return torch.stack(lgs), torch.stack(hids), cache


_ARM = {}


def _arm(name, dt, tokens=None):
    """The fake-quantised native arm of a case in `dt`: (tokens (NEW, B), logits, hidden, cache), teacher-forced with `tokens` (None: its own
    greedy tokens).  Computed once per (case, type) and shared; nothing modifies it."""
    key = (name, dt)
    if key not in _ARM:
        m, x, am, pos = _model(name, dt)
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(ops, "kv_append", _fake_quantising_append(ops.kv_append))
            if tokens is None:
                tokens = m.generate(inputs_embeds=x, attention_mask=am, position_ids=pos, max_new_tokens=NEW).t().contiguous()
            _ARM[key] = (tokens,) + _teacher_forced(m, x, am, pos, tokens, "native")
    return _ARM[key]


@pytest.mark.parametrize("name", MODEL_CASES)
def test_fp32_prefill_and_decode_against_the_fake_quantised_native_arm(name):
    m, x, am, pos = _model(name)
    T = x.shape[1]
    cache = KVCache.for_model(m.model, x.shape[0], T + NEW, kv_format="fp8")
    assert torch.equal(m.model.prefill(x, am, pos, cache), m.model._forward(x, am, pos))          # only what is written to the cache is quantised
    assert cache.len == T and torch.equal(cache.key_mask[:, :T].cpu(), am.cpu().to(torch.uint8))
    tokens, lgs_a, hids_a, cache_a = _arm(name, torch.float32)
    lgs, hids, cache = _teacher_forced(m, x, am, pos, tokens, "fp8")
    parity.close(lgs, lgs_a, 1e-4, f"{name} fp8-cache teacher-forced logits against the fake-quantised native arm")
    parity.close(hids, hids_a, 1e-4, f"{name} fp8-cache teacher-forced hidden against the fake-quantised native arm")
    L = cache.len
    assert L == cache_a.len == T + NEW - 1
    for li in range(len(cache.k_q)):
        # the prefill does not read the cache, so slots [0, T) see identical inputs in every layer; layer 0 sees them in the decode steps too
        upto = L if li == 0 else T
        for q, e, ref in ((cache.k_q, cache.k_e, cache_a.k), (cache.v_q, cache.v_e, cache_a.v)):
            got = _dequant(q[li][:, :, :upto].cpu().contiguous(), e[li][:, :, :upto].cpu().contiguous())
            assert torch.equal(got, ref[li][:, :, :upto].cpu().double()), (name, li)


@pytest.mark.parametrize("dt,tag", [(torch.bfloat16, "bf16"), (torch.float16, "fp16")])
@pytest.mark.parametrize("name", [n for n in MODEL_CASES if n in C.DH128])
def test_16bit_drift_is_the_fake_quantised_native_arms(name, dt, tag):
    """The project's 1.5 x convention: under teacher forcing with the fp32 arm's tokens, the fp8-cache run's logits are at most 1.5 x as far
    from the fp32 arm's logits as the same-type native arm's are, in max-rel and in rms-rel."""
    tokens, ref, _, _ = _arm(name, torch.float32)
    m, x, am, pos = _model(name, dt)
    arm = _arm(name, dt, tokens)[1]
    lgs = _teacher_forced(m, x, am, pos, tokens, "fp8")[0]
    ours, theirs = parity.measure(lgs.float(), ref), parity.measure(arm.float(), ref)
    _log(f"{name} {tag} teacher-forced logits against the fp32 arm: fp8-cache max-rel, native-arm max-rel, ratio, fp8-cache rms-rel, native-arm rms-rel, ratio",
         ours[0], theirs[0], ours[0] / theirs[0], ours[1], theirs[1], ours[1] / theirs[1])
    assert ours[0] <= 1.5 * theirs[0] and ours[1] <= 1.5 * theirs[1], (ours, theirs)


# ---- the loop -------------------------------------------------------------------------------------------------------------------------------
def _check_loop(m, x, am, pos):
    out = m.generate(inputs_embeds=x, attention_mask=am, position_ids=pos, max_new_tokens=NEW, return_dict_in_generate=True, output_logits=True,
                     kv_cache="fp8")
    own = _teacher_forced(m, x, am, pos, out.sequences.t().contiguous(), "fp8")[0]
    assert torch.equal(own, out.logits.transpose(0, 1))                # the loop's logits are the teacher-forced logits under its own tokens
    V = own.shape[-1]
    lowest = torch.where(own == own.max(dim=-1, keepdim=True).values, torch.arange(V, device=own.device), V).min(dim=-1).values
    assert torch.equal(out.sequences.t(), lowest)
    return out


@pytest.mark.parametrize("name,dt", [("tiny_left", torch.float32), ("gqa_dh128", torch.bfloat16), ("mqa_dh128_left", torch.float16)])
def test_generate_with_an_fp8_cache_is_its_own_teacher_forced_run(name, dt):
    m, x, am, pos = _model(name, dt)
    full = _check_loop(m, x, am, pos)
    kw = dict(max_new_tokens=NEW, return_dict_in_generate=True, output_logits=True, kv_cache="fp8")
    for b in range(x.shape[0]):                                        # a sequence alone generates what it generates in the batch
        one = m.generate(inputs_embeds=x[b:b + 1], attention_mask=am[b:b + 1], position_ids=pos[b:b + 1], **kw)
        assert torch.equal(one.sequences[0], full.sequences[b]) and torch.equal(one.logits[0], full.logits[b])


def test_fp8_cache_together_with_fp8_weights():
    kw, lc, seed, x, am, pos, _, _ = C.case_inputs("dh128")
    m = SetokimLlamaPrefill(kw)
    m.load_state_dict(O.init_llama_weights(lc, seed=seed), strict=True)
    m = m.to(device=DEV, dtype=torch.bfloat16).eval().quantize_fp8_()
    assert m.weight_format == "fp8_e4m3"
    x, am, pos = x.to(DEV), am.to(DEV), pos.to(DEV)
    out = _check_loop(m, x, am, pos)
    native = m.generate(inputs_embeds=x, attention_mask=am, position_ids=pos, max_new_tokens=NEW, return_dict_in_generate=True, output_logits=True)
    assert torch.equal(native.logits[:, 0], out.logits[:, 0])          # step 0 is the prefill, which the cache's format does not touch


def test_eos_still_pads_and_stops_early_with_an_fp8_cache():
    m, x, am, pos = _model("tiny_left")
    kw = dict(inputs_embeds=x, attention_mask=am, position_ids=pos, max_new_tokens=NEW, kv_cache="fp8")
    tokens = m.generate(**kw).t().cpu()                                # (NEW, B), unconstrained
    n, B = tokens.shape
    s, b = next((s, b) for s in range(1, n - 1) for b in range(B) if int(tokens[s, b]) not in tokens[:s, b].tolist())      # a token new to its sequence
    eos, pad = int(tokens[s, b]), 99
    exp, first = _expected_with_eos(tokens, {eos}, pad)
    assert first[b] == s and (exp[b, s + 1:] == pad).all()
    assert torch.equal(m.generate(eos_token_id=eos, pad_token_id=pad, **kw).cpu(), exp)
    every = sorted({int(t) for t in tokens[2]})                        # every sequence has finished by step 2: the loop ends there
    exp2, first2 = _expected_with_eos(tokens, set(every), every[0])
    got2 = m.generate(eos_token_id=every, **kw).cpu()
    assert max(first2) <= 2 and got2.shape[1] == max(first2) + 1 and torch.equal(got2, exp2)


# ---- memory and non-interference ----------------------------------------------------------------------------------------------------------------
_LAYER_CALLS = ["setok_rmsnorm", "setok_linear", "setok_rope_gqa", "setok_kv_append", "setok_attention_decode_gqa", "setok_linear", "setok_rmsnorm",
                "setok_linear", "setok_swiglu_pairs", "setok_linear"]                  # one layer of a decode step, as LlamaModel.decode_step issued it before the fp8 cache existed


def _step_calls(m, x, am, pos, kv_format, monkeypatch):
    cache = KVCache.for_model(m.model, x.shape[0], x.shape[1] + 2, kv_format=kv_format)
    m.model.prefill(x, am, pos, cache)
    names, real = [], _lib.call
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "call", lambda name, *a, **k: (names.append(name), real(name, *a, **k))[1])
        m.model.decode_step(torch.zeros(x.shape[0], x.shape[2], dtype=x.dtype, device=DEV), cache)
    return names


def test_cache_bytes_and_the_calls_of_a_decode_step(monkeypatch):
    m, x, am, pos = _model("gqa_dh128", torch.bfloat16)
    layers, B, cap = len(m.model.layers), 3, 77
    c = KVCache.for_model(m.model, B, cap, kv_format="fp8")
    assert c.nbytes() == 2 * layers * B * m.model.num_kv_heads * cap * (m.model.head_dim + 1)
    assert all(t.is_cuda and not t.any() for t in c.k_q + c.k_e + c.v_q + c.v_e)
    assert KVCache.for_model(m.model, B, cap).nbytes() == 2 * layers * B * m.model.num_kv_heads * cap * m.model.head_dim * 2
    x = x.to(torch.bfloat16)
    native = _step_calls(m, x, am, pos, "native", monkeypatch)
    assert native == _LAYER_CALLS * layers + ["setok_rmsnorm"]         # exactly the calls of a native step before this format existed
    fp8 = _step_calls(m, x, am, pos, "fp8", monkeypatch)
    swap = {"setok_kv_append": "setok_kv_append_fp8", "setok_attention_decode_gqa": "setok_attention_decode_gqa_fp8kv"}
    assert fp8 == [swap.get(n, n) for n in native] and fp8 != native
