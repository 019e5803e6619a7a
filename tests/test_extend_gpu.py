"""Extending a filled KV cache by several tokens on a real MI355X, through the C ABI: setok_attention_extend_gqa against fp64 and against its
neighbours (the decode kernel, the causal prefill), `LlamaModel.extend` against HuggingFace's teacher-forced states (tests/golden/generate.npz),
`generate(prefill_chunk=)` against HuggingFace's tokens, and `generate(past=)` against a fresh `generate` over the whole conversation.
`pytest -m gpu`."""
import os

import numpy as np
import pytest
import torch

import golden_io
import llama_bwd_cases as C
import parity
import setok_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from setok_amd import ops
    from setok_amd.generation import GenerateOutput, GenerationState, KVCache
    from setok_amd.llama import SetokimLlamaPrefill

DEV = "cuda"
def _define(name):
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return int(re.search(r"#define\s+" + name + r"\s+(\d+)", open(os.path.join(root, "include", "setok_hip.h")).read()).group(1))


CH = _define("SETOK_EXTEND_CHUNK")                 # the header's chunk length: the pairs sit on ITS edges
SP = _define("SETOK_EXTEND_SPAN") * CH             # slots per partial of the 4-wave MFMA kernel (head dim 128, 16 bits, G * Tn > 32)
PAIRS = [(0, 5), (1, 1), (5, 3), (31, 2), (32, 33), (CH - 1, 2), (CH, 1), (CH - 8, 17), (1000, 7), (300, 130)]      # (len0, Tn)
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _log(label, *nums):
    path = os.environ.get("SETOK_PARITY_LOG")
    if path:
        test = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]
        with open(path, "a") as f:
            f.write(f"{test}\t{label}\t" + "\t".join(f"{n:.3e}" for n in nums) + "\n")
    print(label, *[f"{n:.3e}" for n in nums])


def _tol(dt, Dh):
    """tests/test_generate_gpu.py::_tol's, restated: 3e-6 in fp32; 1e-2 at head dim 128 and 2e-2 below it in 16 bits.  The arithmetic and its
    rounding points are the decode kernel's: fp32 scores and softmax, the probabilities and the output rounded to the element type."""
    if dt == torch.float32:
        return 3e-6
    return 1e-2 if Dh == 128 else 2e-2


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------------
def _extend_problem(dt, H, Hkv, Dh, len0, Tn, cap, seed, later_from=None):
    """Four sequences: all keys; left-padded with a hole inside the new chunk; every old slot masked and holes in the new chunk (rows 0, 3, 6, ..
    masked: row 0 is a masked query whose earlier keys are all masked); fully masked.  NaN sits in every slot that counts for no query: the masked
    slots and the slots >= len0 + Tn.  With `later_from` = s the keys and values of queries >= s (slots >= len0 + s) are scaled by 1e3: for the rows
    below s they are keys of LATER queries, and a causal leak into one of those rows is an error of the order of 1e3 instead of one inside the tolerance."""
    B, n = 4, len0 + Tn
    q = _rand(B * Tn, (H + 2 * Hkv) * Dh, seed=seed).to(dt)
    k, v = _rand(B, Hkv, cap, Dh, seed=seed + 1).to(dt), _rand(B, Hkv, cap, Dh, seed=seed + 2).to(dt)
    mask = torch.zeros(B, cap, dtype=torch.uint8)
    mask[0, :n] = 1
    mask[1, n // 3:n] = 1                          # left padding
    if Tn >= 3:
        mask[1, len0 + Tn // 2] = 0                # ... and a hole inside the new chunk
    mask[2, len0:n] = (torch.arange(Tn) % 3 != 0).to(torch.uint8)
    mask[:, n:] = 1                                # (mask bytes past len0 + Tn are not a licence to read)
    if later_from is not None:
        k[:, :, len0 + later_from:n] *= 1e3
        v[:, :, len0 + later_from:n] *= 1e3
    dead = (mask == 0)[:, None, :, None].expand(B, Hkv, cap, Dh).clone()
    dead[:, :, n:] = True
    k, v = k.masked_fill(dead, float("nan")), v.masked_fill(dead, float("nan"))
    return q, k, v, mask


def _extend_ref(q, k, v, mask, H, Hkv, Dh, len0, Tn):
    """fp64: query i of sequence b counts slot j iff j <= len0 + i and mask[b, j] != 0; a query with no counted key gets zeros."""
    B, n = k.shape[0], len0 + Tn
    qq = q[:, :H * Dh].double().reshape(B, Tn, H, Dh)
    kk = k[:, :, :n].double().nan_to_num(0.0).repeat_interleave(H // Hkv, dim=1)
    vv = v[:, :, :n].double().nan_to_num(0.0).repeat_interleave(H // Hkv, dim=1)
    s = torch.einsum("bihd,bhjd->bhij", qq, kk) * Dh ** -0.5
    counts = mask[:, None, None, :n].bool() & (torch.arange(n)[None, :] <= len0 + torch.arange(Tn)[:, None])[None, None]
    p = torch.softmax(s.masked_fill(~counts, float("-inf")), -1).nan_to_num(0.0)
    return torch.einsum("bhij,bhjd->bihd", p, vv).reshape(B * Tn, H * Dh)


def _extend(q, k, v, mask, H, Tn, len0, Dh):
    return ops.attention_extend(q.to(DEV), k.to(DEV), v.to(DEV), mask.to(DEV), H, Tn, len0, Dh ** -0.5)


def _check_extend(dt, H, Hkv, Dh, pairs):
    tol = _tol(dt, Dh)
    for len0, Tn in pairs:
        q, k, v, mask = _extend_problem(dt, H, Hkv, Dh, len0, Tn, len0 + Tn + 5, seed=100 + len0 + Tn)
        got = _extend(q, k, v, mask, H, Tn, len0, Dh).cpu()
        ref = _extend_ref(q, k, v, mask, H, Hkv, Dh, len0, Tn)
        assert torch.isfinite(got.float()).all(), (len0, Tn)
        err = _rel(got, ref)
        print(f"extend {dt} H={H} Hkv={Hkv} Dh={Dh} len0={len0} Tn={Tn}: max-rel {err:.2e} (tol {tol:.0e})")
        assert err < tol, (len0, Tn, err)
        rows = got.reshape(4, Tn, H * Dh).float()
        assert float(rows[3].abs().max()) == 0.0, (len0, Tn)              # no key at all -> zeros
        assert float(rows[2, 0].abs().max()) == 0.0, (len0, Tn)           # a masked query row whose earlier keys are all masked -> zeros
        if Tn < 2:
            continue
        s = (Tn + 1) // 2                                                 # the later queries' keys and values x 1e3: rows below s must not notice
        q, k, v, mask = _extend_problem(dt, H, Hkv, Dh, len0, Tn, len0 + Tn + 5, seed=100 + len0 + Tn, later_from=s)
        got2 = _extend(q, k, v, mask, H, Tn, len0, Dh).cpu().reshape(4, Tn, H * Dh)[:, :s]
        assert torch.isfinite(got2.float()).all(), (len0, Tn)
        err2 = _rel(got2, ref.reshape(4, Tn, H * Dh)[:, :s])
        print(f"   ... rows < {s} with the later keys / values x 1e3: max-rel {err2:.2e}")
        assert err2 < tol, (len0, Tn, err2)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("H,Hkv", [(2, 2), (4, 2), (8, 1)])          # MHA, GQA G = 2, MQA G = 8
@pytest.mark.parametrize("Dh", [16, 64, 128])
def test_attention_extend_against_fp64(dt, H, Hkv, Dh):
    """The (len0, Tn) pairs: the chunk edge between the old keys and the new, the chunk edge inside the new rows, more than one 32-row tile,
    G * Tn not a multiple of 32, the thin verify shape."""
    _check_extend(dt, H, Hkv, Dh, PAIRS)


@pytest.mark.parametrize("dt,Dh", [(torch.bfloat16, 40), (torch.float16, 96)])
@pytest.mark.parametrize("H,Hkv", [(2, 2), (4, 2), (8, 1)])
def test_attention_extend_head_dims_of_the_generic_path(dt, Dh, H, Hkv):
    _check_extend(dt, H, Hkv, Dh, PAIRS)


# (len0, Tn) for the 4-wave MFMA path, whose partials are SP slots long: the span edge between the old keys and the new; the span edge inside the new
# rows; at G = 8, (SP - 40, 64) has a workgroup (rows of queries 0 .. 15) whose second span lies wholly above its rows next to workgroups that reach into
# it, and (SP - 8, 17) a wave in that position inside a workgroup; two and three spans merged
SPAN_PAIRS = [(SP - 1, 5), (SP - 8, 17), (SP - 40, 64), (SP, 33), (1000, 40), (2 * SP - 3, 40)]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("H,Hkv", [(8, 1), (4, 2), (2, 2)])
def test_attention_extend_across_spans_of_the_mfma_path(dt, H, Hkv):
    """Head dim 128 in 16 bits with G * Tn > 32 and len0 + Tn > SP: more than one partial per row on the path that spans SETOK_EXTEND_SPAN chunks
    (every pair at G = 8; at G = 2 and 1 the pairs with fewer rows take the one-wave kernel at these lengths, which is worth running too).  The same
    checks as above: fp64, zeros where nothing counts, NaN in the dead slots, the later queries' keys and values x 1e3."""
    G = H // Hkv
    spanning = [(len0, Tn) for len0, Tn in SPAN_PAIRS if G * Tn > 32 and len0 + Tn > SP]
    assert ops.EXTEND_CHUNK == CH and len(spanning) >= (6 if G == 8 else 4), spanning
    _check_extend(dt, H, Hkv, 128, SPAN_PAIRS)


def _decode_ref(q, k, v, mask, H, Hkv, Dh, n):
    return _extend_ref(q, k, v, mask, H, Hkv, Dh, n - 1, 1)


@pytest.mark.parametrize("dt,H,Hkv,Dh", [(torch.float32, 4, 2, 16), (torch.bfloat16, 8, 1, 128), (torch.float16, 4, 2, 128), (torch.bfloat16, 4, 2, 64)])
def test_extend_of_one_row_and_the_decode_kernel_agree_with_fp64(dt, H, Hkv, Dh):
    """Tn = 1 and setok_attention_decode_gqa over the same cache both sit within the tolerance of the fp64 answer.  They are NOT required to be
    bit-equal: the decode kernel cuts the keys into chunks of 128 and per-wave slices, the extend kernel into chunks of 256 and (at head dim 128 in 16
    bits) MFMA key tiles of 32, so the summation orders differ."""
    for len0 in (5, CH - 1, CH, 1000):
        q, k, v, mask = _extend_problem(dt, H, Hkv, Dh, len0, 1, len0 + 4, seed=300 + len0)
        ref = _decode_ref(q, k, v, mask, H, Hkv, Dh, len0 + 1)
        ext = _extend(q, k, v, mask, H, 1, len0, Dh)
        dec = ops.attention_decode(q.to(DEV), k.to(DEV), v.to(DEV), mask.to(DEV), H, len0 + 1, Dh ** -0.5)
        assert _rel(ext, ref) < _tol(dt, Dh) and _rel(dec, ref) < _tol(dt, Dh), (len0, _rel(ext, ref), _rel(dec, ref))


@pytest.mark.parametrize("dt,H,Hkv,Dh,T", [(torch.float32, 6, 2, 16, 37), (torch.bfloat16, 4, 2, 128, 300), (torch.float16, 4, 1, 128, 129),
                                           (torch.bfloat16, 4, 2, 64, 70)])
def test_extend_from_an_empty_cache_and_the_causal_prefill_agree_with_fp64(dt, H, Hkv, Dh, T):
    """With len0 = 0 every row of setok_attention_extend_gqa and of setok_attention_causal_gqa over the same T sits within the tolerance of the fp64
    answer.  NOT bit-equal: the prefill runs one online softmax over all key tiles, the extend kernel one per chunk of 256 and a merge."""
    B = 3
    qkv = _rand(B * T, (H + 2 * Hkv) * Dh, seed=7).to(dt)
    km = torch.ones(B, T, dtype=torch.uint8)
    km[1, :T // 4] = 0
    km[2, T // 2:T - 1] = 0
    dq = qkv.to(DEV)
    pre = ops.attention_causal(dq, km.reshape(-1).to(DEV), B, T, H, Dh, Dh ** -0.5, Hkv)
    k, v = torch.zeros(B, Hkv, T + 4, Dh, dtype=dt, device=DEV), torch.zeros(B, Hkv, T + 4, Dh, dtype=dt, device=DEV)
    ops.kv_append(dq, k, v, T, H, 0)
    mask = torch.zeros(B, T + 4, dtype=torch.uint8)
    mask[:, :T] = km
    ext = ops.attention_extend(dq, k, v, mask.to(DEV), H, T, 0, Dh ** -0.5)
    ref = _extend_ref(qkv, k.cpu(), v.cpu(), mask, H, Hkv, Dh, 0, T)
    assert _rel(pre, ref) < _tol(dt, Dh) and _rel(ext, ref) < _tol(dt, Dh), (_rel(pre, ref), _rel(ext, ref))
    unseen = ref.reshape(B, T, -1)[1, :T // 4]                            # the left padding's rows see no key: zeros in both
    assert float(unseen.abs().max()) == 0.0 and float(ext.reshape(B, T, -1)[1, :T // 4].float().abs().max()) == 0.0


@pytest.mark.parametrize("dt,H,Hkv,Dh", [(torch.bfloat16, 8, 2, 128), (torch.float16, 2, 2, 128), (torch.float32, 4, 2, 16), (torch.bfloat16, 4, 2, 40)])
def test_attention_extend_invariance(dt, H, Hkv, Dh):
    """A sequence's output bits depend on its own q, keys, values, mask, len0 and Tn only: not on the batch, not on the cache's capacity, not on the run."""
    _invariance(dt, H, Hkv, Dh, 1000, 9)


@pytest.mark.parametrize("dt,H,Hkv", [(torch.bfloat16, 8, 2), (torch.float16, 2, 2)])
def test_attention_extend_invariance_across_spans(dt, H, Hkv):
    """The same on the 4-wave MFMA path with three partials per row (G * Tn > 32, len0 + Tn > 2 SP)."""
    _invariance(dt, H, Hkv, 128, 2 * SP + 100, 40)


def _invariance(dt, H, Hkv, Dh, len0, Tn):
    B = 5
    cap = len0 + Tn + 3
    g = torch.Generator().manual_seed(9)
    q = torch.randn(B * Tn, (H + 2 * Hkv) * Dh, generator=g).to(dt).to(DEV)
    k, v = torch.randn(B, Hkv, cap, Dh, generator=g).to(dt).to(DEV), torch.randn(B, Hkv, cap, Dh, generator=g).to(dt).to(DEV)
    mask = (torch.rand(B, cap, generator=g) > 0.2).to(torch.uint8).to(DEV)
    run = lambda q_, k_, v_, m_: ops.attention_extend(q_, k_, v_, m_, H, Tn, len0, Dh ** -0.5)
    full = run(q, k, v, mask)
    assert torch.equal(full, run(q, k, v, mask))                                                            # two runs
    b = 2
    alone = run(q[b * Tn:(b + 1) * Tn].contiguous(), k[b:b + 1].contiguous(), v[b:b + 1].contiguous(), mask[b:b + 1].contiguous())
    assert torch.equal(alone, full[b * Tn:(b + 1) * Tn])                                                    # alone == inside a batch of 5
    k2, v2 = torch.zeros(B, Hkv, 2 * cap, Dh, dtype=dt, device=DEV), torch.zeros(B, Hkv, 2 * cap, Dh, dtype=dt, device=DEV)
    k2[:, :, :cap], v2[:, :, :cap] = k, v
    m2 = torch.zeros(B, 2 * cap, dtype=torch.uint8, device=DEV)
    m2[:, :cap] = mask
    assert torch.equal(run(q, k2, v2, m2), full)                                                            # cap == 2 * cap


# ---- the model -------------------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def _model(name, dt=torch.float32):
    """(model on the device in `dt`, x, am, pos on the device): the seeded case of tests/llama_bwd_cases.py."""
    kw, lc, seed, x, am, pos, _, _ = C.case_inputs(name)
    key = (name, dt)
    if key not in _MODELS:
        if name == "7bdims":
            _MODELS.clear()                                            # (2.6 GB in fp32: one at a time)
        m = SetokimLlamaPrefill(kw)
        m.load_state_dict(O.init_llama_weights(lc, seed=seed), strict=True)
        _MODELS[key] = m.to(device=DEV, dtype=dt).eval()
    return _MODELS[key], x.to(DEV), am.to(DEV), pos.to(DEV)


def _golden(golden_dir, name):
    z = golden_io.load(os.path.join(golden_dir, "generate.npz"))
    return {k.split(":", 1)[1]: _t(z[k]) for k in z.files if k.startswith(name + ":")}


def _prefill(m, x, am, pos, room):
    cache = KVCache.for_model(m.model, x.shape[0], x.shape[1] + room)
    m.model.prefill(x, am, pos, cache)
    return cache


def _logits(m, hidden):
    """hidden (B, Tn, D) -> (Tn, B, V), the goldens' layout."""
    B, Tn, D = hidden.shape
    return ops.linear(hidden.reshape(B * Tn, D).contiguous(), m.lm_head.weight.detach().contiguous()).reshape(B, Tn, -1).transpose(0, 1)


@pytest.mark.parametrize("name", list(C.LLAMA_CASES))
def test_fp32_extend_against_hf(golden_dir, name):
    """The goldens' hidden[j] / logits[j] are HuggingFace's states after the prompt plus tokens[:j].  A prefill and ONE extend over the embeddings of
    tokens[0 : n - 1] must give hidden[1:] and logits[1:] within 1e-4 — the bound decode_step is held to — and so must the same rows fed as
    extend, decode_step, extend."""
    m, x, am, pos = _model(name)
    g = _golden(golden_dir, name)
    n, B = g["tokens"].shape
    T, D = x.shape[1], x.shape[2]
    emb = m.model.embed_tokens.weight.detach()[g["tokens"][:n - 1].t().to(DEV)]          # (B, n - 1, D)
    cache = _prefill(m, x, am, pos, n)
    hid = m.model.extend(emb, cache)
    assert hid.shape == (B, n - 1, D) and cache.len == T + n - 1
    assert torch.equal(cache.key_mask[:, T:T + n - 1].cpu(), torch.ones(B, n - 1, dtype=torch.uint8))
    parity.close(hid.transpose(0, 1), g["hidden"][1:], 1e-4, f"{name} extend hidden")
    parity.close(_logits(m, hid), g["logits"][1:], 1e-4, f"{name} extend logits")
    a = min(5, n - 3)                                                  # 7bdims has n = 4: extend(1), decode_step, extend(1)
    cache2 = _prefill(m, x, am, pos, n)
    parts = [m.model.extend(emb[:, :a], cache2), m.model.decode_step(emb[:, a].contiguous(), cache2)[:, None], m.model.extend(emb[:, a + 1:], cache2)]
    hid2 = torch.cat(parts, dim=1)
    assert cache2.len == T + n - 1 and torch.equal(cache2.next_pos, cache.next_pos)
    parity.close(hid2.transpose(0, 1), g["hidden"][1:], 1e-4, f"{name} extend / decode_step / extend hidden")
    parity.close(_logits(m, hid2), g["logits"][1:], 1e-4, f"{name} extend / decode_step / extend logits")


@pytest.mark.parametrize("dt,tag", [(torch.bfloat16, "bf16"), (torch.float16, "fp16")])
@pytest.mark.parametrize("name", list(C.DH128))
def test_16bit_extend_drift_against_hfs_own_16bit_run(golden_dir, name, dt, tag):
    """The yardstick of test_generate_gpu.py: the logits of one extend over HF's fp32 tokens are at most 1.5 x as far from the fp32 golden as
    HuggingFace's OWN teacher-forced run in that type, in max-rel and in rms-rel."""
    m, x, am, pos = _model(name, dt)
    g = _golden(golden_dir, name)
    n, B = g["tokens"].shape
    emb = m.model.embed_tokens.weight.detach()[g["tokens"][:n - 1].t().to(DEV)]
    lgs = _logits(m, m.model.extend(emb, _prefill(m, x, am, pos, n)))
    ours, hf = parity.measure(lgs.float(), g["logits"][1:]), parity.measure(g["logits_" + tag][1:], g["logits"][1:])
    _log(f"{name} {tag} extend logits: GPU max-rel, HF max-rel, ratio, GPU rms-rel, HF rms-rel, ratio",
         ours[0], hf[0], ours[0] / hf[0], ours[1], hf[1], ours[1] / hf[1])
    assert ours[0] <= 1.5 * hf[0] and ours[1] <= 1.5 * hf[1], (ours, hf)


@pytest.mark.parametrize("name", ["gqa_tiny_left", "gqa_dh128"])
def test_fp32_extend_by_a_ragged_masked_chunk_against_hf(golden_dir, name):
    """tests/golden/extend.npz (make_golden_extend.py): HuggingFace's final-norm states and logits for ONE forward over a seeded chunk appended to
    `past_key_values`, whose mask has a hole, a shorter sequence and (with three sequences) a masked first row.  The attended rows within 1e-4."""
    import sys
    sys.path.insert(0, golden_dir)
    from make_golden_extend import TN, chunk_inputs
    z = golden_io.load(os.path.join(golden_dir, "extend.npz"))
    m, x, am, pos = _model(name)
    chunk, cm = chunk_inputs(name)
    assert np.array_equal(z[name + ":chunk_mask"], cm.numpy()) and cm.shape[1] == TN
    cache = _prefill(m, x, am, pos, TN)
    before = cache.next_pos.clone()
    hid = m.model.extend(chunk.to(DEV), cache, cm.to(DEV))
    live = cm.bool()
    assert torch.equal(cache.key_mask[:, x.shape[1]:].cpu(), cm.to(torch.uint8)) and torch.equal((cache.next_pos - before).cpu(), cm.sum(1))
    parity.close(hid.cpu()[live], _t(z[name + ":hidden"])[live], 1e-4, f"{name} ragged chunk hidden")
    parity.close(_logits(m, hid).transpose(0, 1).cpu()[live], _t(z[name + ":logits"])[live], 1e-4, f"{name} ragged chunk logits")


# ---- chunked prefill ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_left", "gqa_tiny_left", "dh128"])
def test_fp32_chunked_prefill_generates_hfs_tokens(golden_dir, name):
    """generate(prefill_chunk=c) returns HuggingFace's token at every step (the goldens' top-2 margins are >= 5e-4 of max|logit| against a 1e-4 logit
    bound); c >= T and c = None are the unchunked path, bit for bit."""
    m, x, am, _ = _model(name)
    g = _golden(golden_dir, name)
    n, B = g["tokens"].shape
    T = x.shape[1]
    kw = dict(inputs_embeds=x, attention_mask=am, max_new_tokens=n, return_dict_in_generate=True, output_logits=True)
    plain = m.generate(**kw)
    assert torch.equal(plain.sequences.cpu(), g["tokens"].t())
    for c in (1, 7, 64):
        out = m.generate(prefill_chunk=c, **kw)
        assert torch.equal(out.sequences.cpu(), g["tokens"].t()), c
        parity.close(out.logits.transpose(0, 1), g["logits"], 1e-4, f"{name} prefill_chunk={c} logits")
    for c in (T, T + 9):
        out = m.generate(prefill_chunk=c, **kw)
        assert torch.equal(out.sequences, plain.sequences) and torch.equal(out.logits, plain.logits), c


def test_bf16_chunked_prefill_tokens_are_the_argmax_of_its_own_logits():
    m, x, am, _ = _model("dh128_left", torch.bfloat16)
    for c in (7, 32):
        out = m.generate(inputs_embeds=x, attention_mask=am, max_new_tokens=12, prefill_chunk=c, return_dict_in_generate=True, output_logits=True)
        lg = out.logits
        assert torch.isfinite(lg.float()).all()
        V = lg.shape[-1]
        lowest = torch.where(lg == lg.max(dim=-1, keepdim=True).values, torch.arange(V, device=lg.device), V).min(dim=-1).values
        assert torch.equal(out.sequences, lowest), c


# ---- two turns ---------------------------------------------------------------------------------------------------------------------------------
def _pick_eos(tokens, n1):
    """An eos id with which one sequence finishes at step 3 and another never does within n1 steps (test_eos_pads... picks the same way)."""
    B = tokens.shape[1]
    for b in range(B):
        eos = int(tokens[3, b])
        first = [next((j for j in range(n1) if int(tokens[j, o]) == eos), n1) for o in range(B)]
        if first[b] == 3 and n1 in first:
            return eos, first
    raise AssertionError("no eos id of the goldens finishes one sequence at step 3 and leaves another running")


@pytest.mark.parametrize("name", ["tiny_left", "gqa_dh128"])
def test_two_turns_equal_one_fresh_generate_over_the_conversation(golden_dir, name):
    """The definition of `past`: turn 2 from the returned state gives the tokens, and within 1e-4 the logits, of a FRESH generate over
    [prompt | that sequence's tokens up to its eos | turn 2] with the concatenated mask and default positions — the path the other tests hold to HF."""
    m, x, am, _ = _model(name)
    tokens = _golden(golden_dir, name)["tokens"]
    B, T, D = x.shape
    n1, n2, L2, pad = 8, 6, 6, 99
    eos, first = _pick_eos(tokens, n1)
    turn1 = dict(inputs_embeds=x, attention_mask=am, max_new_tokens=n1, eos_token_id=eos, pad_token_id=pad, return_dict_in_generate=True, return_past=True)
    out1 = m.generate(cache_capacity=T + n1 + 1 + L2 + n2, **turn1)
    state = out1.past
    assert isinstance(state, GenerationState) and state.pending.shape == (B,) and state.pending.dtype == torch.int64
    seq1 = out1.sequences.cpu()
    real = [min(f + 1, seq1.shape[1]) for f in first]                      # tokens up to and including the first eos
    assert state.pending.cpu().tolist() == [int(seq1[b, -1]) if real[b] == seq1.shape[1] else -1 for b in range(B)]
    w_e = m.model.embed_tokens.weight.detach()
    am2 = torch.ones(B, L2, dtype=torch.long, device=DEV)
    am2[B - 1, L2 - 2:] = 0                                                # ragged: the last sequence's turn is two rows shorter
    fresh_kw = dict(max_new_tokens=n2, return_dict_in_generate=True, output_logits=True)
    for seed in range(40, 60):
        turn = _rand(B, L2, D, seed=seed).to(DEV)
        conv = torch.zeros(B, T + n1 + L2, D, device=DEV)
        cam = torch.zeros(B, T + n1 + L2, dtype=torch.long, device=DEV)
        for b in range(B):
            conv[b, :T], cam[b, :T] = x[b], am[b]
            conv[b, T:T + real[b]], cam[b, T:T + real[b]] = w_e[seq1[b, :real[b]].to(DEV)], 1
            conv[b, T + n1:], cam[b, T + n1:] = turn[b], am2[b]
        fresh = m.generate(inputs_embeds=conv, attention_mask=cam, **fresh_kw)
        top2 = fresh.logits.float().topk(2, dim=-1).values
        margin = float(((top2[..., 0] - top2[..., 1]) / fresh.logits.float().abs().amax(dim=-1)).min())
        if margin >= 5e-4:                                                 # token equality is only meaningful above the logit bound
            break
    else:
        raise AssertionError("no seeded turn with a top-1 / top-2 margin >= 5e-4 at every step")
    out2 = m.generate(past=state, inputs_embeds=turn, attention_mask=am2, return_past=True, **fresh_kw)
    assert out2.past.cache is state.cache                                  # the reserved capacity sufficed: no new cache
    assert torch.equal(out2.sequences, fresh.sequences)
    parity.close(out2.logits, fresh.logits, 1e-4, f"{name} turn 2 logits")
    # without the reservation the continuation moves to a larger cache: the same slots, the same bits; turn 2 through windows: within the bound
    state_b = m.generate(**turn1).past
    assert state_b.cache.cap == T + n1
    out2b = m.generate(past=state_b, inputs_embeds=turn, attention_mask=am2, return_past=True, **fresh_kw)
    assert out2b.past.cache is not state_b.cache and state_b.cache.len == T + out1.sequences.shape[1] - 1      # the old state was left as it was
    assert torch.equal(out2b.sequences, out2.sequences) and torch.equal(out2b.logits, out2.logits)
    out2c = m.generate(past=m.generate(**turn1).past, inputs_embeds=turn, attention_mask=am2, prefill_chunk=4, **fresh_kw)
    assert torch.equal(out2c.sequences, fresh.sequences)
    parity.close(out2c.logits, fresh.logits, 1e-4, f"{name} turn 2 in windows of 4, logits")


# ---- fp8 weights -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tn", [8, 40])                                    # B * Tn = 16 <= FP8W_MAX_M (the streaming GEMM) and 80 > it (the dequantise scratch)
def test_extend_on_fp8_weights_equals_the_prefill_over_the_concatenation(Tn):
    """After quantize_fp8_() the model is exactly a Llama on a weight grid, so the fresh path on the same quantised model is the reference: prefill of
    the first T - Tn columns + extend of the rest against the prefill over all T, within the fp32 1e-4 bound."""
    name = "dh128_left"
    kw, lc, seed, x, am, _, _, _ = C.case_inputs(name)
    m = SetokimLlamaPrefill(kw)
    m.load_state_dict(O.init_llama_weights(lc, seed=seed), strict=True)
    m = m.to(DEV).eval().quantize_fp8_()
    x, am = x.to(DEV), am.to(DEV)
    B, T, D = x.shape
    assert (B * Tn <= ops.FP8W_MAX_M) == (Tn == 8)
    pos = (am.cumsum(-1) - 1).masked_fill(am == 0, 1)
    whole = m.model._forward(x, am, pos)
    cache = KVCache.for_model(m.model, B, T)
    m.model.prefill(x[:, :T - Tn], am[:, :T - Tn], pos[:, :T - Tn], cache)
    hid = m.model.extend(x[:, T - Tn:], cache, am[:, T - Tn:])
    live = am[:, T - Tn:].bool()                                           # (a padding row's state means nothing on either path)
    assert cache.len == T and bool(live[0].all())
    parity.close(hid[live], whole[:, T - Tn:][live], 1e-4, f"fp8 weights, extend of {Tn} rows")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_cache_untouched():
    m, x, am, pos = _model("tiny_left")
    B, T, D = x.shape

    def snapshot(c):
        return c.len, c.key_mask.clone(), c.next_pos.clone()

    def unchanged(c, snap):
        return c.len == snap[0] and torch.equal(c.key_mask, snap[1]) and torch.equal(c.next_pos, snap[2])

    f8 = KVCache.for_model(m.model, B, T + 8, kv_format="fp8")
    m.model.prefill(x, am, pos, f8)
    snap = snapshot(f8)
    with pytest.raises(NotImplementedError, match="fp8"):
        m.model.extend(x[:, :3], f8)
    assert unchanged(f8, snap)
    with pytest.raises(NotImplementedError, match="fp8"):
        m.generate(inputs_embeds=x, attention_mask=am, max_new_tokens=2, kv_cache="fp8", prefill_chunk=4)
    cache = _prefill(m, x, am, pos, 4)
    snap = snapshot(cache)
    with pytest.raises(ValueError, match="cap"):
        m.model.extend(x[:, :5], cache)                                    # len + 5 > cap = len + 4
    assert unchanged(cache, snap)
    with pytest.raises(ValueError):
        m.model.extend(x[:B - 1, :2], cache)                               # a B that does not match the cache
    assert unchanged(cache, snap)
    with pytest.raises(ValueError):
        m.model.extend(x[:, :0], KVCache.for_model(m.model, B, 4))         # nothing to extend an empty cache by
    out = m.generate(inputs_embeds=x, attention_mask=am, max_new_tokens=3, return_dict_in_generate=True, return_past=True)
    snap, pend = snapshot(out.past.cache), out.past.pending.clone()
    with pytest.raises(ValueError, match="position_ids"):
        m.generate(past=out.past, inputs_embeds=x[:, :2], position_ids=pos[:, :2], max_new_tokens=2)
    with pytest.raises(ValueError):
        m.generate(past=out.past, inputs_embeds=x[:B - 1, :2], max_new_tokens=2)      # another batch size
    half = SetokimLlamaPrefill(C.LLAMA_CASES["tiny_left"][0]).to(device=DEV, dtype=torch.bfloat16).eval()
    with pytest.raises(ValueError, match="bfloat16"):
        half.generate(past=out.past, inputs_embeds=x[:, :2], max_new_tokens=2)        # another model dtype
    assert unchanged(out.past.cache, snap) and torch.equal(out.past.pending, pend)
    assert isinstance(out, GenerateOutput)
