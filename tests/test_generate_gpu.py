"""KV-cached greedy generation on a real MI355X, all through the C ABI: setok_kv_append, setok_attention_decode_gqa and setok_argmax_rows against
torch references, and `LlamaModel.prefill` / `decode_step` / `SetokimLlamaPrefill.generate` against HuggingFace LlamaForCausalLM's greedy loop with
past_key_values (tests/golden/generate.npz, tests/golden/make_golden_generate.py).  `pytest -m gpu`."""
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
    from setok_amd.generation import GenerateOutput, KVCache
    from setok_amd.llama import SetokimLlamaPrefill

DEV = "cuda"
CHUNK = 128                                        # SETOK_DECODE_CHUNK
LENS = (1, 31, 32, 33, CHUNK - 1, CHUNK, CHUNK + 1, 1000, 2049)
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
    """tests/test_llama_gpu.py::test_attention_causal_with_padding's: 3e-6 in fp32; 1e-2 at head dim 128 and 2e-2 at head dim 64 in 16 bits.  Head dim
    16 in 16 bits has no entry there: it takes the head-dim-64 bound — the error is the rounding of the probabilities and of the output to the
    element type (2^-9 relative each in bf16), which does not grow as the head dim shrinks, while fewer products average it."""
    if dt == torch.float32:
        return 3e-6
    return 1e-2 if Dh == 128 else 2e-2


# ---- ops ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,Dh", [(torch.float32, 16), (torch.bfloat16, 128), (torch.float16, 64), (torch.float32, 24)])
def test_kv_append_writes_its_slots_and_nothing_else(dt, Dh):
    B, T, H, Hkv, cap, pos0 = 2, 3, 4, 2, 9, 2
    qkv = _rand(B * T, (H + 2 * Hkv) * Dh, seed=1).to(dt).to(DEV)
    k0, v0 = _rand(B, Hkv, cap, Dh, seed=2).to(dt).to(DEV), _rand(B, Hkv, cap, Dh, seed=3).to(dt).to(DEV)
    k, v = k0.clone(), v0.clone()
    ops.kv_append(qkv, k, v, T, H, pos0)
    src = qkv.reshape(B, T, H + 2 * Hkv, Dh)
    assert torch.equal(k[:, :, pos0:pos0 + T], src[:, :, H:H + Hkv].transpose(1, 2))          # bit-equal to the source columns
    assert torch.equal(v[:, :, pos0:pos0 + T], src[:, :, H + Hkv:].transpose(1, 2))
    keep = torch.ones(cap, dtype=torch.bool, device=DEV)
    keep[pos0:pos0 + T] = False
    assert torch.equal(k[:, :, keep], k0[:, :, keep]) and torch.equal(v[:, :, keep], v0[:, :, keep])      # every other slot unchanged


def _decode_problem(dt, H, Hkv, Dh, n, cap, seed):
    """Four sequences: all keys, left-padded, right-padded, fully masked.  Slots at or past n — and the masked slots below it — hold NaN: a kernel
    that lets one of them reach the output fails."""
    B = 4
    qkv = _rand(B, (H + 2 * Hkv) * Dh, seed=seed).to(dt)
    k, v = _rand(B, Hkv, cap, Dh, seed=seed + 1).to(dt), _rand(B, Hkv, cap, Dh, seed=seed + 2).to(dt)
    mask = torch.zeros(B, cap, dtype=torch.uint8)
    mask[0, :n] = 1
    mask[1, n // 3:n] = 1                          # left padding
    mask[2, :n - n // 4] = 1                       # right padding
    mask[:, n:] = 1                                # (mask bytes past len are not a licence to read)
    dead = (mask == 0)[:, None, :, None].expand(B, Hkv, cap, Dh).clone()
    dead[:, :, n:] = True
    k, v = k.masked_fill(dead, float("nan")), v.masked_fill(dead, float("nan"))
    return qkv, k, v, mask


def _decode_ref(qkv, k, v, mask, H, Hkv, Dh, n):
    B = qkv.shape[0]
    q = qkv[:, :H * Dh].double().reshape(B, H, Dh)
    kk = k[:, :, :n].double().nan_to_num(0.0).repeat_interleave(H // Hkv, dim=1)
    vv = v[:, :, :n].double().nan_to_num(0.0).repeat_interleave(H // Hkv, dim=1)
    s = torch.einsum("bhd,bhjd->bhj", q, kk) * Dh ** -0.5
    s = s.masked_fill(~mask[:, None, :n].bool(), float("-inf"))
    p = torch.softmax(s, -1).nan_to_num(0.0)
    return torch.einsum("bhj,bhjd->bhd", p, vv).reshape(B, H * Dh)


def _decode(qkv, k, v, mask, H, n, Dh):
    return ops.attention_decode(qkv.to(DEV), k.to(DEV), v.to(DEV), mask.to(DEV), H, n, Dh ** -0.5)


def _decode_cases():
    """Head dims 16, 64, 128 in every element type and head grouping (MHA, GQA G = 2 and 4, MQA G = 4 and 8), and the lane layouts those leave out:
    head dims 8 and 32 in fp32 (2 and 8 lanes per row), 32 and 256 in the 16-bit types (4 and 32 lanes), each with one and eight query heads per
    workgroup.  The ids are those of three stacked parametrisations (Dh, then H-Hkv, then dt)."""
    cases = [(dt, H, Hkv, Dh) for Dh in (16, 64, 128) for H, Hkv in [(2, 2), (4, 2), (8, 2), (4, 1), (8, 1)] for dt in DTYPES]
    cases += [(dt, H, Hkv, Dh) for dt in DTYPES for Dh in ((8, 32) if dt == torch.float32 else (32, 256)) for H, Hkv in [(2, 2), (8, 1)]]
    return [pytest.param(dt, H, Hkv, Dh, id=f"{Dh}-{H}-{Hkv}-dt{DTYPES.index(dt)}") for dt, H, Hkv, Dh in cases]


@pytest.mark.parametrize("dt,H,Hkv,Dh", _decode_cases())
def test_attention_decode_against_fp64(dt, H, Hkv, Dh):
    tol = _tol(dt, Dh)
    for n in LENS:
        qkv, k, v, mask = _decode_problem(dt, H, Hkv, Dh, n, n + 5, seed=100 + n)
        got = _decode(qkv, k, v, mask, H, n, Dh).cpu()
        ref = _decode_ref(qkv, k, v, mask, H, Hkv, Dh, n)
        assert torch.isfinite(got.float()).all(), n
        err = _rel(got, ref)
        print(f"decode {dt} H={H} Hkv={Hkv} Dh={Dh} len={n}: max-rel {err:.2e} (tol {tol:.0e})")
        assert err < tol, (n, err)
        assert float(got[3].float().abs().max()) == 0.0, n                # no key at all -> zeros


@pytest.mark.parametrize("dt,Dh", [(torch.float32, 24), (torch.bfloat16, 40), (torch.float16, 96)])
def test_attention_decode_head_dims_outside_the_lane_layouts(dt, Dh):
    """Every head dim setok_attention_causal_gqa accepts (a multiple of 8) works: these take the generic kernel."""
    H, Hkv = 4, 2
    for n in (1, 33, CHUNK + 1, 300):
        qkv, k, v, mask = _decode_problem(dt, H, Hkv, Dh, n, n + 3, seed=200 + n)
        got = _decode(qkv, k, v, mask, H, n, Dh).cpu()
        assert _rel(got, _decode_ref(qkv, k, v, mask, H, Hkv, Dh, n)) < _tol(dt, Dh), n
        assert float(got[3].float().abs().max()) == 0.0


@pytest.mark.parametrize("dt,H,Hkv,Dh,T", [(torch.float32, 6, 2, 16, 37), (torch.bfloat16, 4, 2, 128, 300), (torch.float16, 4, 1, 128, 129),
                                           (torch.bfloat16, 4, 2, 64, 70)])
def test_decode_and_the_prefills_last_row_agree_with_fp64(dt, H, Hkv, Dh, T):
    """The last query row of setok_attention_causal_gqa over T keys and the decode kernel over the same T cached keys both sit within the
    tolerance of the fp64 answer.  They are NOT required to be bit-equal: the prefill accumulates over key tiles of 32 in MFMA order, the decode
    kernel over chunks of 128 cut into per-wave slices, so the summation orders differ."""
    B = 3
    qkv = _rand(B * T, (H + 2 * Hkv) * Dh, seed=7).to(dt)
    km = torch.ones(B, T, dtype=torch.uint8)
    km[1, :T // 4] = 0
    km[2, T // 2:T - 1] = 0                        # (the last token stays attended)
    dq = qkv.to(DEV)
    pre = ops.attention_causal(dq, km.reshape(-1).to(DEV), B, T, H, Dh, Dh ** -0.5, Hkv).reshape(B, T, H * Dh)[:, -1]
    k, v = torch.zeros(B, Hkv, T + 4, Dh, dtype=dt, device=DEV), torch.zeros(B, Hkv, T + 4, Dh, dtype=dt, device=DEV)
    ops.kv_append(dq, k, v, T, H, 0)
    mask = torch.zeros(B, T + 4, dtype=torch.uint8)
    mask[:, :T] = km
    last = dq.reshape(B, T, -1)[:, -1].contiguous()
    dec = ops.attention_decode(last, k, v, mask.to(DEV), H, T, Dh ** -0.5)
    ref = _decode_ref(last.cpu(), k.cpu(), v.cpu(), mask, H, Hkv, Dh, T)
    assert _rel(pre, ref) < _tol(dt, Dh) and _rel(dec, ref) < _tol(dt, Dh)


@pytest.mark.parametrize("dt,H,Hkv,Dh", [(torch.bfloat16, 8, 2, 128), (torch.float16, 2, 2, 128), (torch.float32, 4, 2, 16), (torch.bfloat16, 4, 2, 40)])
def test_attention_decode_invariance(dt, H, Hkv, Dh):
    """A sequence's output bits depend on its own q, keys, values, mask and len only: not on the batch, not on the cache's capacity, not on the run."""
    n, cap, B = 1000, 1003, 5
    g = torch.Generator().manual_seed(9)
    qkv = torch.randn(B, (H + 2 * Hkv) * Dh, generator=g).to(dt).to(DEV)
    k, v = torch.randn(B, Hkv, cap, Dh, generator=g).to(dt).to(DEV), torch.randn(B, Hkv, cap, Dh, generator=g).to(dt).to(DEV)
    mask = (torch.rand(B, cap, generator=g) > 0.2).to(torch.uint8).to(DEV)
    full = ops.attention_decode(qkv, k, v, mask, H, n, Dh ** -0.5)
    assert torch.equal(full, ops.attention_decode(qkv, k, v, mask, H, n, Dh ** -0.5))                       # two runs
    b = 2
    alone = ops.attention_decode(qkv[b:b + 1].contiguous(), k[b:b + 1].contiguous(), v[b:b + 1].contiguous(), mask[b:b + 1].contiguous(), H, n, Dh ** -0.5)
    assert torch.equal(alone[0], full[b])                                                                   # alone == inside a batch of 5
    k2, v2 = torch.zeros(B, Hkv, 2 * cap, Dh, dtype=dt, device=DEV), torch.zeros(B, Hkv, 2 * cap, Dh, dtype=dt, device=DEV)
    k2[:, :, :cap], v2[:, :, :cap] = k, v
    m2 = torch.zeros(B, 2 * cap, dtype=torch.uint8, device=DEV)
    m2[:, :cap] = mask
    assert torch.equal(ops.attention_decode(qkv, k2, v2, m2, H, n, Dh ** -0.5), full)                       # cap == 2 * cap


@pytest.mark.parametrize("dt", DTYPES)
def test_argmax_rows_lowest_index_of_the_maximum(dt):
    rows, V = 7, 32003
    x = _rand(rows, V, seed=11).to(dt)
    top = float(x.float().max()) + 1.0
    x[0, 5] = top; x[0, 31000] = top                                   # planted ties: the lowest index wins
    x[1, 0] = top; x[1, V - 1] = top
    x[2, V - 1] = top                                                  # the last column alone
    x[3, 255] = top; x[3, 256] = top; x[3, 257] = top                  # neighbours that different threads scan
    want = torch.where(x == x.max(dim=1, keepdim=True).values, torch.arange(V)[None], V).min(dim=1).values
    assert want[:4].tolist() == [5, 0, V - 1, 255]
    got = ops.argmax_rows(x.to(DEV))
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), want)
    if dt == torch.float32:                                            # (16-bit rows of 32003 draws tie at the maximum: torch.argmax names no winner there)
        uniq = (x == x.max(dim=1, keepdim=True).values).sum(1) == 1
        assert torch.equal(got.cpu()[uniq], torch.argmax(x, dim=1)[uniq]) and int(uniq.sum()) >= 3
    wide = torch.full((rows, V + 5), 1e4, dtype=dt)                     # a row stride larger than V: the columns behind V are never read
    wide[:, :V] = x
    assert torch.equal(ops.argmax_rows(wide.to(DEV)[:, :V]).cpu(), want)
    assert torch.equal(ops.argmax_rows(x.to(DEV)), got)                # deterministic


# ---- model ------------------------------------------------------------------------------------------------------------------------------
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


def _teacher_forced(m, x, am, pos, tokens):
    """Prefill + decode_step feeding `tokens` (n, B): (logits (n, B, V), hidden (n, B, D)) — the states and logits that predict token j."""
    n, B = tokens.shape
    T = x.shape[1]
    cache = KVCache.for_model(m.model, B, T + n)
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
    return torch.stack(lgs), torch.stack(hids)


@pytest.mark.parametrize("name", list(C.LLAMA_CASES))
def test_fp32_prefill_decode_and_generate_against_hf(golden_dir, name):
    m, x, am, pos = _model(name)
    g = _golden(golden_dir, name)
    n, B = g["tokens"].shape
    T = x.shape[1]
    cache = KVCache.for_model(m.model, B, T + n)
    assert torch.equal(m.model.prefill(x, am, pos, cache), m.model._forward(x, am, pos))          # the cached prefill keeps _forward's bits
    assert cache.len == T and torch.equal(cache.key_mask[:, :T].cpu(), am.cpu().to(torch.uint8))
    lgs, hids = _teacher_forced(m, x, am, pos, g["tokens"])
    parity.close(lgs, g["logits"], 1e-4, f"{name} teacher-forced logits")
    parity.close(hids, g["hidden"], 1e-4, f"{name} teacher-forced hidden")
    out = m.generate(inputs_embeds=x, attention_mask=am, position_ids=pos, max_new_tokens=n, return_dict_in_generate=True,
                     output_hidden_states=True, output_logits=True)
    assert isinstance(out, GenerateOutput) and out.sequences.dtype == torch.int64
    assert torch.equal(out.sequences.cpu(), g["tokens"].t())                                        # HF's token at every step of every sequence
    assert out.hidden_states.shape == (B, n, x.shape[2]) and out.logits.shape == (B, n, g["logits"].shape[2])
    assert torch.equal(out.logits.transpose(0, 1), lgs) and torch.equal(out.hidden_states.transpose(0, 1), hids)
    plain = m.generate(inputs_embeds=x, attention_mask=am, position_ids=pos, max_new_tokens=n)
    assert torch.equal(plain, out.sequences)


@pytest.mark.parametrize("dt,tag", [(torch.bfloat16, "bf16"), (torch.float16, "fp16")])
@pytest.mark.parametrize("name", list(C.DH128))
def test_16bit_drift_against_hfs_own_16bit_run_and_the_loop(golden_dir, name, dt, tag):
    """The yardstick of the llama_bwd tests: under teacher forcing with HF's fp32 tokens, the GPU's 16-bit logits are at most 1.5 x as far from the
    fp32 golden as HuggingFace's OWN run in that type, in max-rel and in rms-rel.  Then the loop: generate()'s tokens are the argmax of the
    teacher-forced logits under its own tokens, and those logits are bit-equal to the loop's (the same kernels on the same inputs)."""
    m, x, am, pos = _model(name, dt)
    g = _golden(golden_dir, name)
    n, B = g["tokens"].shape
    lgs, _ = _teacher_forced(m, x, am, pos, g["tokens"])
    ours, hf = parity.measure(lgs.float(), g["logits"]), parity.measure(g["logits_" + tag], g["logits"])
    _log(f"{name} {tag} teacher-forced logits: GPU max-rel, HF max-rel, ratio, GPU rms-rel, HF rms-rel, ratio",
         ours[0], hf[0], ours[0] / hf[0], ours[1], hf[1], ours[1] / hf[1])
    assert ours[0] <= 1.5 * hf[0] and ours[1] <= 1.5 * hf[1], (ours, hf)
    out = m.generate(inputs_embeds=x, attention_mask=am, position_ids=pos, max_new_tokens=n, return_dict_in_generate=True, output_logits=True)
    own, _ = _teacher_forced(m, x, am, pos, out.sequences.t().contiguous())
    assert torch.equal(own, out.logits.transpose(0, 1))
    V = own.shape[-1]
    lowest = torch.where(own == own.max(dim=-1, keepdim=True).values, torch.arange(V, device=own.device), V).min(dim=-1).values
    assert torch.equal(out.sequences.t(), lowest)


# ---- loop behaviour ------------------------------------------------------------------------------------------------------------------------
def _expected_with_eos(tokens, eos, pad):
    """tokens (n, B) of the unconstrained run -> (B, n') as generate must return them with the eos ids: pad after a sequence's first eos, the loop
    ending with the step at which the last sequence finishes."""
    n, B = tokens.shape
    exp = tokens.t().clone()
    first = []
    for b in range(B):
        hit = [j for j in range(n) if int(tokens[j, b]) in eos]
        first.append(hit[0] if hit else n)
        exp[b, first[-1] + 1:] = pad
    stop = max(first) + 1 if max(first) < n else n
    return exp[:, :stop], first


def test_eos_pads_finished_sequences_and_ends_the_loop_early(golden_dir):
    name = "tiny_left"
    m, x, am, pos = _model(name)
    tokens = _golden(golden_dir, name)["tokens"]
    n, B = tokens.shape
    b = next(b for b in range(B) if int(tokens[3, b]) not in tokens[:3, b].tolist())          # a sequence whose step-3 token is new to it
    eos, pad = int(tokens[3, b]), 99
    exp, first = _expected_with_eos(tokens, {eos}, pad)
    assert first[b] == 3 and exp.shape[1] > 4
    got = m.generate(inputs_embeds=x, attention_mask=am, position_ids=pos, max_new_tokens=n, eos_token_id=eos, pad_token_id=pad).cpu()
    assert torch.equal(got, exp)
    assert got[b, 4:].tolist() == [pad] * (got.shape[1] - 4)                                  # pads from step 4 on
    for o in range(B):
        if first[o] == n:
            assert torch.equal(got[o], tokens[:got.shape[1], o])                              # the others' tokens are unchanged
    every = sorted({int(t) for t in tokens[2]})                                               # every sequence has finished by step 2: the loop ends there
    exp2, first2 = _expected_with_eos(tokens, set(every), every[0])
    got2 = m.generate(inputs_embeds=x, attention_mask=am, position_ids=pos, max_new_tokens=n, eos_token_id=every).cpu()
    assert max(first2) <= 2 and got2.shape[1] == max(first2) + 1 and torch.equal(got2, exp2)  # (pad_token_id defaults to the first eos id)


def test_a_sequence_alone_generates_what_it_generates_in_the_batch(golden_dir):
    name = "dh128_left"
    m, x, am, pos = _model(name, torch.bfloat16)
    kw = dict(max_new_tokens=12, return_dict_in_generate=True, output_logits=True)
    full = m.generate(inputs_embeds=x, attention_mask=am, position_ids=pos, **kw)
    for b in range(x.shape[0]):
        one = m.generate(inputs_embeds=x[b:b + 1], attention_mask=am[b:b + 1], position_ids=pos[b:b + 1], **kw)
        assert torch.equal(one.sequences[0], full.sequences[b]) and torch.equal(one.logits[0], full.logits[b])


def test_generate_from_ids_and_images_equals_generate_from_the_spliced_embeddings():
    """input_ids with IMAGE_TOKEN_INDEX placeholders + images -> encode -> splice -> prefill -> decode, against the same call on the spliced
    embeddings (tokenizer and projector stood in for as test_llama_gpu.py::test_setokim_forward_splices_then_prefills does)."""
    kw = dict(hidden_size=64, intermediate_size=176, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4, vocab_size=100)
    sd = O.init_llama_weights(O.LlamaConfigLite(**kw), seed=11)
    ids, am, _, feats, _ = O.splice_inputs(12, 4, 10, 100, 64)

    class Tower:
        pass

    m = SetokimLlamaPrefill(kw, vision_tower=Tower())
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    m.encode_images = lambda images, **k: [f.to(DEV) for f in feats]
    imgs = torch.zeros(len(feats), 3, 2, 2)
    kwg = dict(max_new_tokens=8, return_dict_in_generate=True, output_logits=True)
    a = m.generate(ids.to(DEV), comp_images=imgs, attention_mask=am.to(DEV), **kwg)
    assert torch.equal(m.generate(inputs=ids.to(DEV), images=imgs, attention_mask=am.to(DEV), **kwg).sequences, a.sequences)   # the reference's keyword
    _, ram, remb, _ = O.splice_multimodal(ids, None, am, None, feats, sd["model.embed_tokens.weight"])
    assert remb.shape[1] > ids.shape[1]                                                       # the splice lengthened the prompt
    b = m.generate(inputs_embeds=remb.to(DEV), attention_mask=ram.to(DEV), **kwg)
    assert a.sequences.shape == (4, 8) and torch.equal(a.sequences, b.sequences)
    assert _rel(a.logits, b.logits) < 1e-5
    _, ref = O.llama_forward(sd, O.LlamaConfigLite(**kw), remb, ram, None)                    # step 0 is the prefill's last attended position
    last = (ram * torch.arange(ram.shape[1])[None]).max(1).values
    assert _rel(a.logits[:, 0].cpu(), ref[torch.arange(4), last]) < 1e-4


def test_generate_refuses_what_it_does_not_implement():
    kw = dict(hidden_size=64, intermediate_size=176, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=4, vocab_size=100)
    torch.manual_seed(0)
    x = torch.randn(2, 9, 64, device=DEV)
    m = SetokimLlamaPrefill(kw).to(DEV).eval()
    with pytest.raises(NotImplementedError, match="greedy"):
        m.generate(inputs_embeds=x, max_new_tokens=2, do_sample=True)
    with pytest.raises(NotImplementedError, match="greedy"):
        m.generate(inputs_embeds=x, max_new_tokens=2, temperature=0.1, top_p=10.0)            # the reference's defaults
    with pytest.raises(TypeError):
        m.generate(inputs_embeds=x, max_new_tokens=2, no_such_argument=1)
    w = SetokimLlamaPrefill(dict(kw, sliding_window=12)).to(DEV).eval()
    w.load_state_dict(m.state_dict())
    with pytest.raises(NotImplementedError, match="sliding_window"):
        w.generate(inputs_embeds=x, max_new_tokens=4)                                         # 9 + 4 > 12
    assert torch.equal(w.generate(inputs_embeds=x, max_new_tokens=3), m.generate(inputs_embeds=x, max_new_tokens=3))      # a window that covers it is plain attention
    with pytest.raises(NotImplementedError):
        SetokimLlamaPrefill(dict(kw, attention_bias=True))                                    # what the prefill refuses stays refused


@pytest.mark.grad
def test_generate_records_no_graph():
    kw = dict(hidden_size=64, intermediate_size=176, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=4, vocab_size=100)
    torch.manual_seed(0)
    m = SetokimLlamaPrefill(kw).to(DEV).train()
    assert torch.is_grad_enabled() and all(p.requires_grad for p in m.parameters())
    x = torch.randn(2, 9, 64, device=DEV, requires_grad=True)
    out = m.generate(inputs_embeds=x, max_new_tokens=3, return_dict_in_generate=True, output_hidden_states=True, output_logits=True)
    for t in (out.sequences, out.hidden_states, out.logits):
        assert t.grad_fn is None and not t.requires_grad
