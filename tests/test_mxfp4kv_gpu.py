"""The MXFP4 KV cache on a real MI355X (include/setok_hip.h, "MXFP4 KV cache"): setok_kv_append_mxfp4 against the CPU oracle of the storage contract
(tests/mxfp4_cases.py) bit for bit, setok_attention_decode_gqa_mxfp4kv and setok_attention_extend_gqa_mxfp4kv against the fp64 attention over the
dequantised cache K', V', and `prefill` / `decode_step` / `extend` / `generate(kv_cache="mxfp4")` against a FAKE-QUANTISED NATIVE ARM: the
unchanged native path whose appended cache slots are round-tripped through the oracle's quantiser on the CPU.  K', V' are exact in every element
type and the arithmetic on them is the native kernels', so no test here carries a tolerance for quantisation error.  `pytest -m gpu`."""
import pytest
import torch

import llama_bwd_cases as C
import mxfp4_cases as M
import mxfp4kv_cases as K
import parity
import setok_oracle as O
from test_extend_gpu import _extend_problem, _extend_ref
from test_fp8kv_gpu import _LAYER_CALLS, _step_calls, _teacher_forced
from test_generate_gpu import DEV, DTYPES, _decode_ref, _expected_with_eos, _log, _model, _rand, _rel, _tol

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from setok_amd import ops
    from setok_amd.generation import BeamSearch, KVCache, LookupDrafter
    from setok_amd.llama import SetokimLlamaPrefill

CH = K.define("SETOK_DECODE_CHUNK_MXFP4KV")
XC = K.define("SETOK_EXTEND_CHUNK")
LENS = (1, 31, 32, 33, CH - 1, CH, CH + 1, 2 * CH + 37)
PAIRS = [(0, 5), (1, 1), (31, 2), (XC - 1, 2), (XC, 1), (XC - 8, 17)]      # (len0, Tn)
NEW = 8
MODEL_CASES = ("dh128", "gqa_dh128", "mqa_dh128_left", "dh32_left")


# ---- operators ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("Dh", [32, 64, 128, 96])
def test_kv_append_mxfp4_equals_the_oracle_bit_for_bit(dt, Dh):
    B, T, H, Hkv, cap, pos0 = 2, 3, 4, 2, 9, 2
    rows = M.quantizer_matrix(B * T * 2 * Hkv, Dh, dt)                 # zeros, both clamps, saturation, every tie in both signs, -0, 20-octave neighbours
    rows[5, 1], rows[5, 3], rows[5, Dh - 1] = float("nan"), float("inf"), float("-inf")
    qkv = _rand(B * T, H + 2 * Hkv, Dh, seed=1).to(dt)
    qkv[:, H:] = rows.reshape(B * T, 2 * Hkv, Dh)                      # row (b, t, j): j < Hkv the k head j, else the v head j - Hkv
    g = torch.Generator().manual_seed(2)
    q0 = [torch.randint(0, 256, (B, Hkv, cap, Dh // 2), generator=g, dtype=torch.uint8).to(DEV) for _ in range(2)]
    s0 = [torch.randint(0, 256, (B, Hkv, cap, Dh // 32), generator=g, dtype=torch.uint8).to(DEV) for _ in range(2)]
    k_q, v_q, k_s, v_s = q0[0].clone(), q0[1].clone(), s0[0].clone(), s0[1].clone()
    ops.kv_append_mxfp4(qkv.reshape(B * T, -1).to(DEV), k_q, k_s, v_q, v_s, T, H, pos0)
    wq, ws = M.quantize_rows(rows)
    wq, ws = wq.reshape(B, T, 2 * Hkv, Dh // 2), ws.reshape(B, T, 2 * Hkv, Dh // 32)
    live = ws[ws != M.NAN_SCALE]
    assert int((ws == M.NAN_SCALE).sum()) == (2 if Dh > 32 else 1) and live.min() == M.BIAS + M.E_MIN and live.max() == M.BIAS + M.E_MAX
    assert torch.equal(k_q[:, :, pos0:pos0 + T].cpu(), wq[:, :, :Hkv].transpose(1, 2))
    assert torch.equal(v_q[:, :, pos0:pos0 + T].cpu(), wq[:, :, Hkv:].transpose(1, 2))
    assert torch.equal(k_s[:, :, pos0:pos0 + T].cpu(), ws[:, :, :Hkv].transpose(1, 2))
    assert torch.equal(v_s[:, :, pos0:pos0 + T].cpu(), ws[:, :, Hkv:].transpose(1, 2))
    keep = torch.ones(cap, dtype=torch.bool, device=DEV)
    keep[pos0:pos0 + T] = False                                        # every other slot: nibbles and scale bytes unchanged
    assert torch.equal(k_q[:, :, keep], q0[0][:, :, keep]) and torch.equal(v_q[:, :, keep], q0[1][:, :, keep])
    assert torch.equal(k_s[:, :, keep], s0[0][:, :, keep]) and torch.equal(v_s[:, :, keep], s0[1][:, :, keep])


def _check_attention(dt, H, Hkv, Dh, n, cap, seed, label):
    qkv, k_q, k_s, v_q, v_s, mask = K.decode_problem(dt, H, Hkv, Dh, n, cap, seed)
    got = ops.attention_decode_mxfp4kv(qkv.to(DEV), k_q.to(DEV), k_s.to(DEV), v_q.to(DEV), v_s.to(DEV), mask.to(DEV), H, n, Dh ** -0.5).cpu()
    ref = _decode_ref(qkv, K.dequant(k_q, k_s), K.dequant(v_q, v_s), mask, H, Hkv, Dh, n)      # (dead slots: NaN or 2^-127 garbage, masked in the reference)
    err, tol = _rel(got, ref), _tol(dt, Dh)
    _log(f"mxfp4kv decode{label} {dt} H={H} Hkv={Hkv} Dh={Dh} len={n}: max-rel, tol", err, tol)
    assert torch.isfinite(got.float()).all(), n
    assert err < tol, (n, err, tol)
    assert float(got[3].float().abs().max()) == 0.0, n                 # no key at all -> zeros


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("H,Hkv", [(2, 2), (4, 2), (8, 2), (4, 1), (8, 1)])
@pytest.mark.parametrize("Dh", [32, 64, 128])                          # 2, 4 and 8 lanes per row
def test_attention_decode_mxfp4kv_against_fp64_on_the_dequantised_cache(dt, H, Hkv, Dh):
    for n in LENS:
        _check_attention(dt, H, Hkv, Dh, n, n + 5, 100 + n, "")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("H,Hkv", [(2, 2), (4, 2), (8, 2), (4, 1), (8, 1)])
def test_attention_decode_mxfp4kv_head_dim_96_takes_the_generic_kernel(dt, H, Hkv):
    for n in LENS:
        _check_attention(dt, H, Hkv, 96, n, n + 3, 200 + n, " (generic)")


def test_a_counted_slot_with_a_nan_block_gives_nan_and_a_dead_one_does_not():
    """A 0xFF scale byte in a slot that counts is a NaN in the cache and reaches the output, as a NaN in a native cache would; the same byte in a
    masked slot, or past len, is discarded."""
    H, Hkv, Dh, n, cap = 4, 2, 64, 40, 48
    for dt in (torch.float32, torch.bfloat16):
        qkv, k_q, k_s, v_q, v_s, mask = K.decode_problem(dt, H, Hkv, Dh, n, cap, 7)
        k_s[0, 1, 5, 1] = 0xFF                                         # sequence 0 (all keys count), key / value head 1: query heads 2 and 3
        got = ops.attention_decode_mxfp4kv(qkv.to(DEV), k_q.to(DEV), k_s.to(DEV), v_q.to(DEV), v_s.to(DEV), mask.to(DEV), H, n, Dh ** -0.5).cpu().float()
        got = got.reshape(4, H, Dh)
        assert torch.isnan(got[0, 2:]).all() and torch.isfinite(got[0, :2]).all() and torch.isfinite(got[1:]).all()


@pytest.mark.parametrize("dt,H,Hkv,Dh", [(torch.bfloat16, 8, 2, 128), (torch.float16, 2, 2, 128), (torch.float32, 4, 2, 32), (torch.bfloat16, 4, 2, 96)])
def test_attention_decode_mxfp4kv_invariance(dt, H, Hkv, Dh):
    """A sequence's output bits depend on its own q, nibbles, scales, mask and len only: not on the batch, not on the capacity, not on the run."""
    n, B = 2 * CH + 37, 5
    cap = n + 3
    g = torch.Generator().manual_seed(9)
    qkv = torch.randn(B, (H + 2 * Hkv) * Dh, generator=g).to(dt).to(DEV)
    k_q, k_s, v_q, v_s = [t.to(DEV) for t in K.cache_rows(B, Hkv, cap, Dh, 10)]
    mask = (torch.rand(B, cap, generator=g) > 0.2).to(torch.uint8).to(DEV)
    run = lambda *a: ops.attention_decode_mxfp4kv(*a, H, n, Dh ** -0.5)
    full = run(qkv, k_q, k_s, v_q, v_s, mask)
    assert torch.equal(full, run(qkv, k_q, k_s, v_q, v_s, mask))                                            # two runs
    b = 2
    alone = run(*[t[b:b + 1].contiguous() for t in (qkv, k_q, k_s, v_q, v_s, mask)])
    assert torch.equal(alone[0], full[b])                                                                   # alone == inside a batch of 5
    def widen(t):                                                      # the slot axis doubled, zeros behind the cache
        dim = 1 if t.dim() == 2 else 2
        w = torch.zeros(t.shape[:dim] + (2 * cap,) + t.shape[dim + 1:], dtype=t.dtype, device=DEV)
        w.narrow(dim, 0, cap).copy_(t)
        return w
    wide = [widen(t) for t in (k_q, k_s, v_q, v_s, mask)]
    assert torch.equal(run(qkv, *wide), full)                                                               # cap == 2 * cap


def _extend_mx(q, k, v, mask, H, Tn, len0, Dh):
    """The extend attention over the oracle's quantisation of k, v (a NaN row — a slot that counts for no query — becomes 0xFF blocks); also K', V'."""
    k_q, k_s = K.quantize_cache(k)
    v_q, v_s = K.quantize_cache(v)
    got = ops.attention_extend_mxfp4kv(q.to(DEV), k_q.to(DEV), k_s.to(DEV), v_q.to(DEV), v_s.to(DEV), mask.to(DEV), H, Tn, len0, Dh ** -0.5).cpu()
    return got, K.dequant(k_q, k_s), K.dequant(v_q, v_s)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("H,Hkv", [(2, 2), (8, 1)])
@pytest.mark.parametrize("Dh", [32, 128])
def test_attention_extend_mxfp4kv_against_fp64_on_the_dequantised_cache(dt, H, Hkv, Dh):
    tol = _tol(dt, Dh)
    for len0, Tn in PAIRS:
        q, k, v, mask = _extend_problem(dt, H, Hkv, Dh, len0, Tn, len0 + Tn + 5, seed=100 + len0 + Tn)
        got, kd, vd = _extend_mx(q, k, v, mask, H, Tn, len0, Dh)
        ref = _extend_ref(q, kd, vd, mask, H, Hkv, Dh, len0, Tn)
        err = _rel(got, ref)
        _log(f"mxfp4kv extend {dt} H={H} Hkv={Hkv} Dh={Dh} len0={len0} Tn={Tn}: max-rel, tol", err, tol)
        assert torch.isfinite(got.float()).all(), (len0, Tn)
        assert err < tol, (len0, Tn, err)
        rows = got.reshape(4, Tn, H * Dh).float()
        assert float(rows[3].abs().max()) == 0.0, (len0, Tn)              # no key at all -> zeros
        assert float(rows[2, 0].abs().max()) == 0.0, (len0, Tn)           # a masked query row whose earlier keys are all masked -> zeros
        if Tn < 2:
            continue
        s = (Tn + 1) // 2                                                 # the later queries' keys and values x 1e3 BEFORE quantising: rows below s must not notice
        q, k, v, mask = _extend_problem(dt, H, Hkv, Dh, len0, Tn, len0 + Tn + 5, seed=100 + len0 + Tn, later_from=s)
        got2 = _extend_mx(q, k, v, mask, H, Tn, len0, Dh)[0].reshape(4, Tn, H * Dh)[:, :s]
        err2 = _rel(got2, ref.reshape(4, Tn, H * Dh)[:, :s])
        _log(f"   ... rows < {s} with the later keys / values x 1e3: max-rel", err2)
        assert torch.isfinite(got2.float()).all(), (len0, Tn)
        assert err2 < tol, (len0, Tn, err2)


# ---- model: the fake-quantised native arm ---------------------------------------------------------------------------------------------------
def _fake_quantising_append(real):
    """ops.kv_append followed by a round trip of the appended slots through the CPU oracle: the native cache then holds K', V'."""
    def append(qkv, k_cache, v_cache, T, H, pos0):
        real(qkv, k_cache, v_cache, T, H, pos0)
        for c in (k_cache, v_cache):
            c[:, :, pos0:pos0 + T] = K.round_trip(c[:, :, pos0:pos0 + T])
    return append


class _arm_path:
    """Inside: the native path is the fake-quantised arm."""
    def __enter__(self):
        self.mp = pytest.MonkeyPatch()
        self.mp.setattr(ops, "kv_append", _fake_quantising_append(ops.kv_append))
    def __exit__(self, *exc):
        self.mp.undo()


_DH32 = {}


def _case(name, dt=torch.float32):
    """test_generate_gpu._model, extended by the head-dim-32 case of mxfp4kv_cases.py."""
    if name != "dh32_left":
        return _model(name, dt)
    kw, sd, x, am, pos = K.dh32_case()
    if dt not in _DH32:
        m = SetokimLlamaPrefill(kw)
        m.load_state_dict(sd, strict=True)
        _DH32[dt] = m.to(device=DEV, dtype=dt).eval()
    return _DH32[dt], x.to(DEV), am.to(DEV), pos.to(DEV)


_ARM = {}


def _arm(name, dt, tokens=None):
    """The fake-quantised native arm of a case in `dt`: (tokens (NEW, B), logits, hidden, cache), teacher-forced with `tokens` (None: its own
    greedy tokens).  Computed once per (case, type) and shared; nothing modifies it."""
    key = (name, dt)
    if key not in _ARM:
        m, x, am, pos = _case(name, dt)
        with _arm_path():
            if tokens is None:
                tokens = m.generate(inputs_embeds=x, attention_mask=am, position_ids=pos, max_new_tokens=NEW).t().contiguous()
            _ARM[key] = (tokens,) + _teacher_forced(m, x, am, pos, tokens, "native")
    return _ARM[key]


@pytest.mark.parametrize("name", MODEL_CASES)
def test_fp32_prefill_and_decode_against_the_fake_quantised_native_arm(name):
    m, x, am, pos = _case(name)
    T = x.shape[1]
    cache = KVCache.for_model(m.model, x.shape[0], T + NEW, kv_format="mxfp4")
    assert torch.equal(m.model.prefill(x, am, pos, cache), m.model._forward(x, am, pos))          # only what is written to the cache is quantised
    assert cache.len == T and torch.equal(cache.key_mask[:, :T].cpu(), am.cpu().to(torch.uint8))
    tokens, lgs_a, hids_a, cache_a = _arm(name, torch.float32)
    lgs, hids, cache = _teacher_forced(m, x, am, pos, tokens, "mxfp4")
    parity.close(lgs, lgs_a, 1e-4, f"{name} mxfp4-cache teacher-forced logits against the fake-quantised native arm")
    parity.close(hids, hids_a, 1e-4, f"{name} mxfp4-cache teacher-forced hidden against the fake-quantised native arm")
    L = cache.len
    assert L == cache_a.len == T + NEW - 1
    for li in range(len(cache.k_q)):
        # the prefill does not read the cache, so slots [0, T) see identical inputs in every layer; layer 0 sees them in the decode steps too
        upto = L if li == 0 else T
        for q, s, ref in ((cache.k_q, cache.k_s, cache_a.k), (cache.v_q, cache.v_s, cache_a.v)):
            got = K.dequant(q[li][:, :, :upto], s[li][:, :, :upto])
            assert torch.equal(got, ref[li][:, :, :upto].cpu().double()), (name, li)


@pytest.mark.parametrize("dt,tag", [(torch.bfloat16, "bf16"), (torch.float16, "fp16")])
@pytest.mark.parametrize("name", [n for n in MODEL_CASES if n in C.DH128])
def test_16bit_drift_is_the_fake_quantised_native_arms(name, dt, tag):
    """The project's 1.5 x convention: under teacher forcing with the fp32 arm's tokens, the mxfp4-cache run's logits are at most 1.5 x as far
    from the fp32 arm's logits as the same-type native arm's are, in max-rel and in rms-rel."""
    tokens, ref, _, _ = _arm(name, torch.float32)
    m, x, am, pos = _case(name, dt)
    arm = _arm(name, dt, tokens)[1]
    lgs = _teacher_forced(m, x, am, pos, tokens, "mxfp4")[0]
    ours, theirs = parity.measure(lgs.float(), ref), parity.measure(arm.float(), ref)
    _log(f"{name} {tag} teacher-forced logits against the fp32 arm: mxfp4-cache max-rel, native-arm max-rel, ratio, mxfp4-cache rms-rel, native-arm rms-rel, ratio",
         ours[0], theirs[0], ours[0] / theirs[0], ours[1], theirs[1], ours[1] / theirs[1])
    assert ours[0] <= 1.5 * theirs[0] and ours[1] <= 1.5 * theirs[1], (ours, theirs)


# ---- the loop -------------------------------------------------------------------------------------------------------------------------------
def _lowest_argmax(lg):
    V = lg.shape[-1]
    return torch.where(lg == lg.max(dim=-1, keepdim=True).values, torch.arange(V, device=lg.device), V).min(dim=-1).values


def _check_loop(m, x, am, pos):
    out = m.generate(inputs_embeds=x, attention_mask=am, position_ids=pos, max_new_tokens=NEW, return_dict_in_generate=True, output_logits=True,
                     kv_cache="mxfp4")
    own = _teacher_forced(m, x, am, pos, out.sequences.t().contiguous(), "mxfp4")[0]
    assert torch.equal(own, out.logits.transpose(0, 1))                # the loop's logits are the teacher-forced logits under its own tokens
    assert torch.equal(out.sequences.t(), _lowest_argmax(own))
    return out


@pytest.mark.parametrize("name,dt", [("dh32_left", torch.float32), ("gqa_dh128", torch.bfloat16), ("mqa_dh128_left", torch.float16)])
def test_generate_with_an_mxfp4_cache_is_its_own_teacher_forced_run(name, dt):
    m, x, am, pos = _case(name, dt)
    x = x.to(dt)
    full = _check_loop(m, x, am, pos)
    kw = dict(max_new_tokens=NEW, return_dict_in_generate=True, output_logits=True, kv_cache="mxfp4")
    for b in range(x.shape[0]):                                        # a sequence alone generates what it generates in the batch
        one = m.generate(inputs_embeds=x[b:b + 1], attention_mask=am[b:b + 1], position_ids=pos[b:b + 1], **kw)
        assert torch.equal(one.sequences[0], full.sequences[b]) and torch.equal(one.logits[0], full.logits[b])


def test_mxfp4_cache_together_with_mxfp4_weights():
    kw, lc, seed, x, am, pos, _, _ = C.case_inputs("dh128")
    m = SetokimLlamaPrefill(kw)
    m.load_state_dict(O.init_llama_weights(lc, seed=seed), strict=True)
    m = m.to(device=DEV, dtype=torch.bfloat16).eval().quantize_mxfp4_()
    assert m.weight_format == "mxfp4_e2m1"
    x, am, pos = x.to(DEV), am.to(DEV), pos.to(DEV)
    out = _check_loop(m, x, am, pos)
    native = m.generate(inputs_embeds=x, attention_mask=am, position_ids=pos, max_new_tokens=NEW, return_dict_in_generate=True, output_logits=True)
    assert torch.equal(native.logits[:, 0], out.logits[:, 0])          # step 0 is the prefill, which the cache's format does not touch


def test_eos_still_pads_and_stops_early_with_an_mxfp4_cache():
    m, x, am, pos = _case("dh32_left")
    kw = dict(inputs_embeds=x, attention_mask=am, position_ids=pos, max_new_tokens=NEW, kv_cache="mxfp4")
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


def test_beam_search_on_an_mxfp4_cache_finds_the_arms_beams():
    m, x, am, pos = _case("mqa_dh128_left")
    kw = dict(inputs_embeds=x, attention_mask=am, position_ids=pos, max_new_tokens=NEW, beams=BeamSearch(3), return_dict_in_generate=True)
    with _arm_path():
        arm = m.generate(**kw)
    out = m.generate(kv_cache="mxfp4", **kw)
    assert torch.equal(out.sequences, arm.sequences)
    rel = float(((out.sequences_scores - arm.sequences_scores).abs() / arm.sequences_scores.abs()).max())
    _log("mqa_dh128_left fp32 beams=3: sequences_scores against the arm's, max relative difference", rel)
    assert rel < 1e-5, rel


def test_cache_bytes_and_the_calls_of_a_decode_step(monkeypatch):
    m, x, am, pos = _model("gqa_dh128", torch.bfloat16)
    layers, B, cap = len(m.model.layers), 3, 77
    c = KVCache.for_model(m.model, B, cap, kv_format="mxfp4")
    assert c.nbytes() == 2 * layers * B * m.model.num_kv_heads * cap * (m.model.head_dim // 2 + m.model.head_dim // 32)
    assert all(t.is_cuda and not t.any() for t in c.k_q + c.k_s + c.v_q + c.v_s)
    x = x.to(torch.bfloat16)
    native = _step_calls(m, x, am, pos, "native", monkeypatch)
    assert native == _LAYER_CALLS * layers + ["setok_rmsnorm"]         # exactly the calls of a native step before this format existed
    fp8 = _step_calls(m, x, am, pos, "fp8", monkeypatch)
    swap8 = {"setok_kv_append": "setok_kv_append_fp8", "setok_attention_decode_gqa": "setok_attention_decode_gqa_fp8kv"}
    assert fp8 == [swap8.get(n, n) for n in native]                    # ... and of an fp8 step
    mx = _step_calls(m, x, am, pos, "mxfp4", monkeypatch)
    swap = {"setok_kv_append": "setok_kv_append_mxfp4", "setok_attention_decode_gqa": "setok_attention_decode_gqa_mxfp4kv"}
    assert mx == [swap.get(n, n) for n in native] and mx != native     # the append and attention names differ, nothing else


# ---- extending the cache: extend, chunked prefill, drafting, turns ----------------------------------------------------------------------------
@pytest.mark.parametrize("name,Tn", [("mqa_dh128_left", 3), ("mqa_dh128_left", 17), ("dh32_left", 3)])
def test_fp32_extend_over_an_mxfp4_cache_against_the_arms_extend(name, Tn):
    m, x, am, pos = _case(name)
    B, T, _ = x.shape
    def run(kv_format):
        cache = KVCache.for_model(m.model, B, T + 2, kv_format=kv_format)
        m.model.prefill(x[:, :T - Tn], am[:, :T - Tn], pos[:, :T - Tn], cache)
        return m.model.extend(x[:, T - Tn:], cache, am[:, T - Tn:]), cache
    with _arm_path():
        ref, cache_a = run("native")
    got, cache = run("mxfp4")
    assert bool(am[:, T - Tn:].all())                                  # (left padding: every new row is attended, so every hidden state means something)
    parity.close(got, ref, 1e-4, f"{name} extend of {Tn} rows over an mxfp4 cache against the arm's extend")
    assert cache.len == cache_a.len == T                               # layer 0's rows see identical inputs: the stored slots are the arm's
    assert torch.equal(K.dequant(cache.k_q[0][:, :, :T], cache.k_s[0][:, :, :T]), cache_a.k[0][:, :, :T].cpu().double())
    assert torch.equal(K.dequant(cache.v_q[0][:, :, :T], cache.v_s[0][:, :, :T]), cache_a.v[0][:, :, :T].cpu().double())


GAP_CASE, GAP_NEW = "mqa_dh128_left", 10       # a case whose greedy logits keep a top-2 gap above 1e-3 of the row's maximum at every step (asserted below)


def _assert_gap(logits, what):
    """Token equality between two summation orders is only meaningful above the logit bound: fail loudly on a near-tie."""
    lg = logits.float()
    top2 = lg.topk(2, dim=-1).values
    gap = float(((top2[..., 0] - top2[..., 1]) / lg.abs().amax(dim=-1)).min())
    _log(f"{what}: smallest top-2 gap relative to the row's maximum", gap)
    assert gap > 1e-3, (what, gap)


def test_fp32_drafting_over_an_mxfp4_cache_emits_the_plain_loops_tokens():
    m, x, am, pos = _case(GAP_CASE)
    kw = dict(inputs_embeds=x, attention_mask=am, position_ids=pos, max_new_tokens=GAP_NEW, kv_cache="mxfp4")
    plain = m.generate(return_dict_in_generate=True, output_logits=True, **kw)
    _assert_gap(plain.logits, f"{GAP_CASE} plain loop over an mxfp4 cache")
    assert torch.equal(m.generate(draft=LookupDrafter(3), **kw), plain.sequences)


def test_fp32_chunked_prefill_over_an_mxfp4_cache_matches_the_arm_with_the_same_chunking():
    m, x, am, _ = _case(GAP_CASE)
    kw = dict(inputs_embeds=x, attention_mask=am, max_new_tokens=GAP_NEW, prefill_chunk=4, return_dict_in_generate=True, output_logits=True)
    with _arm_path():
        arm = m.generate(**kw)
    _assert_gap(arm.logits, f"{GAP_CASE} arm with prefill_chunk=4")
    out = m.generate(kv_cache="mxfp4", **kw)
    assert torch.equal(out.sequences, arm.sequences)
    parity.close(out.logits, arm.logits, 1e-4, f"{GAP_CASE} prefill_chunk=4 over an mxfp4 cache against the arm with the same chunking, logits")
    whole = m.generate(kv_cache="mxfp4", **dict(kw, prefill_chunk=None))
    assert not torch.equal(whole.logits[:, 0], out.logits[:, 0])       # windows attend over the stored, quantised slots: not the unchunked function


def test_a_turn_from_an_mxfp4_state_equals_a_fresh_generate_that_feeds_the_same_windows():
    m, x, am, _ = _case("dh32_left")
    B, T, D = x.shape
    L2, n2 = 5, 6                                                      # the turn [pending | L2 rows] is ONE window of a fresh prefill_chunk=T run (1 + L2 <= T)
    out1 = m.generate(inputs_embeds=x, attention_mask=am, max_new_tokens=1, kv_cache="mxfp4", return_dict_in_generate=True, return_past=True)
    state = out1.past
    assert state.cache.kv_format == "mxfp4" and state.cache.len == T and state.cache.cap == T + 1
    filled = [[t[:, :, :T].clone() for t in layers] for layers in state.cache._fmt.tensors]
    turn = _rand(B, L2, D, seed=77).to(DEV)
    am2 = torch.ones(B, L2, dtype=torch.long, device=DEV)
    am2[B - 1, L2 - 2:] = 0                                            # ragged: the last sequence's turn is two rows shorter
    kw = dict(max_new_tokens=n2, return_dict_in_generate=True, output_logits=True)
    out2 = m.generate(past=state, inputs_embeds=turn, attention_mask=am2, return_past=True, **kw)
    new = out2.past.cache
    assert new is not state.cache and new.kv_format == "mxfp4" and new.cap >= T + 1 + L2 + n2       # no room: the state moved to a larger cache of its format
    for layers, kept in zip(new._fmt.tensors, filled):                 # `grown` keeps every filled slot bit for bit
        for t, k in zip(layers, kept):
            assert torch.equal(t[:, :, :T], k)
    w_e = m.model.embed_tokens.weight.detach()
    conv = torch.cat([x, w_e[out1.sequences[:, 0]][:, None].to(x.dtype), turn], dim=1)
    cam = torch.cat([am, torch.ones(B, 1, dtype=am.dtype, device=DEV), am2], dim=1)
    fresh = m.generate(inputs_embeds=conv, attention_mask=cam, kv_cache="mxfp4", prefill_chunk=T, **kw)
    assert torch.equal(out2.sequences, fresh.sequences) and torch.equal(out2.logits, fresh.logits)


def test_grown_keeps_every_filled_slot_bit_for_bit():
    m, x, am, pos = _case("dh32_left")
    B, T, _ = x.shape
    cache = KVCache.for_model(m.model, B, T + 1, kv_format="mxfp4")
    m.model.prefill(x, am, pos, cache)
    big = cache.grown(3 * T)
    assert big.kv_format == "mxfp4" and big.cap == 3 * T and big.len == T and torch.equal(big.next_pos, cache.next_pos)
    assert torch.equal(big.key_mask[:, :T], cache.key_mask[:, :T]) and not big.key_mask[:, T:].any()
    for new, old in zip(big._fmt.tensors, cache._fmt.tensors):
        for t, o in zip(new, old):
            assert torch.equal(t[:, :, :T], o[:, :, :T]) and not t[:, :, T:].any()
    step = torch.zeros(B, x.shape[2], device=DEV)
    assert torch.equal(m.model.decode_step(step, big), m.model.decode_step(step, cache))          # and decodes like the cache it came from
