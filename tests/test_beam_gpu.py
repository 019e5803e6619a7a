"""Beam search on a real MI355X, all through the C ABI: setok_beam_topk against fp64 torch, setok_kv_reorder against a torch gather, setok_beam_advance
against the per-step state of the torch statement of the rule (tests/beam_cases.py), and `SetokimLlamaPrefill.generate(beams=...)` against
HuggingFace's own `generate(num_beams=...)` (tests/golden/beam.npz, tests/golden/make_golden_beam.py).  `pytest -m gpu`.

Score error of setok_beam_topk.  The bound is 2 x torch's own fp32-against-fp64 error on the same inputs (log_softmax in fp32, then the add) + one fp32
ulp of the score: the kernel rounds where torch's fp32 path rounds, with another order of the sum and another exp / log, hence the factor."""
import os

import numpy as np
import pytest
import torch

import beam_cases as BC
import golden_io
import llama_bwd_cases as LC
import parity
import setok_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from setok_amd import ops
    from setok_amd.generation import BeamSearch, KVCache
    from setok_amd.llama import SetokimLlamaPrefill

DEV = "cuda"
CHUNK = 128                                        # SETOK_DECODE_CHUNK
GRID = 1.0 / 16                                    # a step every element type represents exactly in [8, 16)


# ---- setok_beam_topk ----------------------------------------------------------------------------------------------------------------------------
def _topk_problem(dt, V, n_in, B, C, seed):
    """Logits (B * n_in, V) on `dt`'s grid and running (B, n_in) fp32 whose top C + 1 accumulated scores are >= 1e-3 apart in fp64: min(C + 1, what the
    live rows hold) planted entries 8 + m / 16 (distinct m inside a row) over noise in [-6, 0]; the rows' offsets running - logsumexp are staggered by
    1 / (16 (n_in + 1)) >= 3.6e-3, so planted entries of different rows cannot meet either.  Where there is room, a row per sequence runs at -1e9 and
    an eighth of every row is -inf."""
    g = torch.Generator().manual_seed(seed)
    x = (-6.0 * torch.rand(B, n_in, V, generator=g, dtype=torch.float64)).to(dt).double()
    dead = torch.zeros(B, n_in, dtype=torch.bool)
    if n_in >= 2 and V >= 2 * C:
        dead[torch.arange(B), torch.randint(1, n_in, (B,), generator=g)] = True
    if V >= 4 * C:
        x.masked_fill_(torch.rand(B, n_in, V, generator=g) < 0.125, float("-inf"))
    for b in range(B):
        live = torch.nonzero(~dead[b]).flatten()
        count = min(C + 1, live.numel() * V)
        at = torch.randperm(live.numel() * V, generator=g)[:count]
        rows, cols = live[at // V], at % V
        for j in live.tolist():
            mine = cols[rows == j]
            x[b, j, mine] = 8.0 + torch.randperm(128, generator=g)[:mine.numel()].double() * GRID
    lse = torch.logsumexp(x, dim=-1)
    running = -2.0 - torch.arange(n_in, dtype=torch.float64)[None] * (GRID / (n_in + 1)) + lse
    running = running.masked_fill(dead, -1.0e9).float()
    return x.to(dt).reshape(B * n_in, V), running


def _strided(x, pad):
    """x (rows, V) inside a (rows, V + pad) buffer whose pad columns are NaN."""
    buf = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), dtype=x.dtype, device=DEV)
    buf[:, :x.shape[1]] = x.to(DEV)
    return buf[:, :x.shape[1]]


def _topk_ref(x, running, C):
    """fp64: (score, token, beam, the top C + 1 values) and torch's own fp32 scores at the same places."""
    B, n_in = running.shape
    V = x.shape[1]
    xd, rd = x.to(DEV), running.to(DEV)
    acc = (torch.log_softmax(xd.double(), dim=-1).view(B, n_in, V) + rd.double()[:, :, None]).reshape(B, n_in * V)
    top, idx = torch.topk(acc, min(C + 1, n_in * V), dim=1)
    acc32 = (torch.log_softmax(xd.float(), dim=-1).view(B, n_in, V) + rd[:, :, None]).reshape(B, n_in * V)
    return top[:, :C], idx[:, :C] % V, (idx[:, :C] // V).to(torch.int32), top, acc32.gather(1, idx[:, :C])


TOPK_CASES = [  # (dt, V, n_in, B, C): every value of every axis, V = C included
    (torch.float32, 2, 1, 1, 2), (torch.bfloat16, 9, 2, 3, 9), (torch.float16, 64, 3, 1, 64), (torch.float32, 64, 16, 3, 64),
    (torch.float32, 100, 1, 3, 9), (torch.bfloat16, 100, 3, 1, 2), (torch.float16, 100, 8, 3, 64),
    (torch.float32, 257, 2, 1, 64), (torch.bfloat16, 257, 16, 3, 9), (torch.float16, 257, 1, 1, 2),
    (torch.bfloat16, 32000, 8, 1, 9), (torch.float32, 32000, 3, 3, 64), (torch.float16, 32000, 16, 1, 2),
    (torch.bfloat16, 128256, 16, 1, 64), (torch.float32, 128256, 2, 3, 9), (torch.float16, 128256, 1, 1, 64), (torch.bfloat16, 128256, 3, 3, 2),
]


@pytest.mark.parametrize("case", range(len(TOPK_CASES)), ids=lambda i: "-".join(str(v).replace("torch.", "") for v in TOPK_CASES[i]))
def test_beam_topk_against_fp64_torch(case):
    dt, V, n_in, B, C = TOPK_CASES[case]
    x, running = _topk_problem(dt, V, n_in, B, C, seed=100 + case)
    ref_s, ref_t, ref_b, top, own = _topk_ref(x, running, C)
    live = top[:, 1:] > -1.0e8
    assert float((top[:, :-1] - top[:, 1:])[live].min()) >= 1.0e-3                         # the construction's margin, in fp64
    xs = _strided(x, 8 if case % 2 == 0 else 5)                                            # whole 16-byte pieces / rows that start anywhere
    score, token, beam, status = ops.beam_topk(xs, running.to(DEV), C)
    assert status.tolist() == [0] * B
    assert torch.equal(token, ref_t) and torch.equal(beam, ref_b)
    err_own = float((own.double() - ref_s).abs().max())
    ulp = torch.finfo(torch.float32).eps * 2.0 ** torch.floor(torch.log2(ref_s.abs().clamp_min(1e-30)))
    err = (score.double() - ref_s).abs()
    print(f"beam_topk {TOPK_CASES[case]}: max err {float(err.max()):.3e}  torch fp32 {err_own:.3e}")
    assert bool((err <= 2.0 * err_own + ulp).all()), (float(err.max()), err_own)
    assert bool((score[:, :-1] >= score[:, 1:]).all())
    if B > 1:                                                                               # a sequence alone, from another buffer with another stride
        alone = ops.beam_topk(x[n_in:2 * n_in].to(DEV).contiguous(), running[1:2].to(DEV).contiguous(), C)
        for a, b in zip(alone[:3], (score, token, beam)):
            assert torch.equal(a, b[1:2])


def test_beam_topk_breaks_an_exact_tie_by_the_lower_flat_index():
    g = torch.Generator().manual_seed(5)
    row = torch.randperm(100, generator=g).float() * GRID                                  # distinct values inside a row
    x = torch.stack([row, row, row]).to(DEV)                                               # ... and three identical rows at the same running score
    score, token, beam, status = ops.beam_topk(x, torch.zeros(1, 3, device=DEV), 9)
    order = torch.argsort(row, descending=True)[:3].to(DEV)
    assert torch.equal(token[0], order.repeat_interleave(3)) and beam[0].tolist() == [0, 1, 2] * 3 and status.tolist() == [0]
    assert bool((score[0].view(3, 3) == score[0].view(3, 3)[:, :1]).all())
    y = torch.zeros(1, 300, device=DEV)                                                    # a whole row of ties: the first C indices
    y[0, 7], y[0, 250] = 1.0, 1.0
    _, token, _, _ = ops.beam_topk(y, torch.zeros(1, 1, device=DEV), 6)
    assert token[0].tolist() == [7, 250, 0, 1, 2, 3]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16])
def test_beam_topk_flags_a_bad_row_and_leaves_its_neighbours_alone(dt):
    x, running = _topk_problem(dt, 257, 2, 4, 9, seed=77)
    clean = ops.beam_topk(x.to(DEV), running.to(DEV), 9)
    bad = x.clone()
    bad[2 * 1 + 1, 200] = float("nan")                                                     # sequence 1, row 1
    bad[2 * 3 + 0, 3] = float("inf")                                                       # sequence 3, row 0
    got = ops.beam_topk(bad.to(DEV), running.to(DEV), 9)
    assert got[3].tolist() == [0, 1, 0, 1] and clean[3].tolist() == [0, 0, 0, 0]
    for a, b in zip(got[:3], clean[:3]):
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    minus = x.clone()
    minus[0] = float("-inf")                                                               # a row without a finite entry is bad as well
    assert ops.beam_topk(minus.to(DEV), running.to(DEV), 9)[3].tolist() == [1, 0, 0, 0]


# ---- setok_kv_reorder ---------------------------------------------------------------------------------------------------------------------------
REORDER_CASES = [  # (format, dt, Dh, n, B, layers, Hkv, slot0, slots)
    ("native", torch.float32, 16, 2, 1, 1, 2, 3, 5), ("native", torch.bfloat16, 64, 3, 3, 3, 2, 7, 1), ("native", torch.bfloat16, 128, 4, 1, 2, 1, 60, 130),
    ("native", torch.float32, 128, 8, 3, 2, 2, 4, 0), ("fp8", torch.bfloat16, 128, 8, 3, 2, 2, 60, 130), ("fp8", torch.bfloat16, 16, 3, 1, 1, 2, 5, 5),
    ("fp8", torch.bfloat16, 64, 2, 3, 2, 1, 9, 1), ("fp8", torch.float16, 64, 4, 1, 1, 2, 11, 0),
]


def _mappings(B, n):
    base = (torch.arange(B * n) // n) * n
    i = torch.arange(B * n) % n
    out = {"identity": base + i, "swap": base + torch.where(i < 2, 1 - i, i), "rotation": base + (i + 1) % n, "one parent": base + n - 1}
    wild = (base + (i + 1) % n).clone()
    wild[0], wild[n - 1] = -1, n                                                           # below the group; the first row of the next one (or past the cache)
    out["out of group"] = wild
    return out


@pytest.mark.parametrize("case", range(len(REORDER_CASES)), ids=lambda i: "-".join(str(v).replace("torch.", "") for v in REORDER_CASES[i]))
def test_kv_reorder_against_a_torch_gather(case):
    fmt, dt, Dh, n, B, layers, Hkv, slot0, ns = REORDER_CASES[case]
    cap = slot0 + ns + 9
    assert ns != 130 or slot0 // CHUNK != (slot0 + ns - 1) // CHUNK                        # the long region straddles a decode chunk
    cache = KVCache(layers, B * n, Hkv, cap, Dh, dt, DEV, fmt)
    cache.len = slot0 + ns
    tensors = [t for group in cache._fmt.tensors for t in group]
    assert len(tensors) == layers * (4 if fmt == "fp8" else 2)
    g = torch.Generator().manual_seed(case)
    start = []
    for t in tensors:
        raw = t.view(torch.uint8)
        raw.fill_(0x7f)                                                                    # every byte outside the region: a pattern no copy produces
        width = raw.shape[3] if raw.dim() == 4 else None
        fresh = torch.randint(0, 256, raw[:, :, slot0:slot0 + ns].shape, generator=g, dtype=torch.uint8)
        raw[:, :, slot0:slot0 + ns] = fresh.to(DEV)
        assert width is None or width == Dh * t.element_size()
        start.append(raw.clone())
    for name, src in _mappings(B, n).items():
        for t, s in zip(tensors, start):
            t.view(torch.uint8).copy_(s)
        cache._plan = None                                                                 # a fresh status
        status = cache.reorder(src.to(device=DEV, dtype=torch.int32), slot0, n)
        ok = (src >= (torch.arange(B * n) // n) * n) & (src < (torch.arange(B * n) // n) * n + n)
        assert status.tolist() == (~ok).int().tolist(), name
        take = torch.where(ok, src, torch.arange(B * n)).to(DEV)
        for t, s in zip(tensors, start):
            want = s.clone()
            want[:, :, slot0:slot0 + ns] = s[take][:, :, slot0:slot0 + ns]
            assert torch.equal(t.view(torch.uint8), want), (name, tuple(t.shape))          # the region bit-equal to the gather, every other byte unchanged


# ---- setok_beam_advance -------------------------------------------------------------------------------------------------------------------------
def _case(golden_dir, name):
    z = golden_io.load(os.path.join(golden_dir, "beam.npz"))
    g = {k.split(":", 1)[1]: torch.from_numpy(np.asarray(z[k])) for k in z.files if k.startswith(name + ":")}
    seed, n, es, eos0, eos1, steps = (int(v) for v in g["spec"])
    g.update(n=n, es={v: k for k, v in BC.ES_CODE.items()}[es], eos=[eos0, eos1], steps=steps, lp=float(g["length_penalty"]))
    g["sd"] = {k[2:]: v for k, v in g.items() if isinstance(k, str) and k.startswith("w:")}
    return g


@pytest.mark.parametrize("name", list(BC.CASES))
def test_beam_advance_follows_the_reference_state_step_by_step(golden_dir, name):
    g = _case(golden_dir, name)
    n, B = g["n"], BC.B
    state = ops.BeamState(B, n, BC.N_NEW, DEV)
    eos = torch.tensor(g["eos"], dtype=torch.int64, device=DEV)
    status = torch.zeros(B, dtype=torch.int32, device=DEV)
    for s in range(g["steps"]):
        tr = {k[6:]: v[s] for k, v in g.items() if isinstance(k, str) and k.startswith("trace:")}
        tok, src, summary = ops.beam_advance(tr["cand_score"].to(DEV), tr["cand_token"].to(DEV), tr["cand_beam"].to(torch.int32).to(DEV), status, state,
                                             eos, s, g["lp"], g["es"])
        what = (name, s)
        assert summary.tolist() == [int(tr["go_on"]), 0], what
        assert torch.equal(tok.cpu(), tr["next_token"]) and torch.equal(src.cpu().long(), tr["src_row"]), what
        assert torch.equal(state.run_score.cpu(), tr["run"]) and torch.equal(state.fin_score.cpu(), tr["fin_score"]), what
        assert torch.equal(state.fin_flag.cpu().bool(), tr["fin_flag"]) and torch.equal(state.heur.cpu().bool(), tr["heur"]), what
        for got, key in ((state.fin_len, "fin_len"), (state.fin_parent, "fin_parent"), (state.fin_token, "fin_token")):
            assert torch.equal(got.cpu().long(), tr[key]), (what, key)
        assert torch.equal(state.bp_token[s].cpu(), tr["next_token"]) and torch.equal(state.bp_parent[s].cpu().long() + (torch.arange(B * n) // n) * n, tr["src_row"])
    assert ops.beam_advance(tr["cand_score"].to(DEV), tr["cand_token"].to(DEV), tr["cand_beam"].to(torch.int32).to(DEV), torch.tensor([0, 1, 0], dtype=torch.int32, device=DEV),
                            ops.BeamState(B, n, BC.N_NEW, DEV), eos, 0, g["lp"], g["es"])[2].tolist()[1] == 1      # a status of setok_beam_topk reaches the summary


# ---- generate(beams=...) ------------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def _fixture_model(golden_dir, name, dt=torch.float32):
    g = _case(golden_dir, name)
    if (name, dt) not in _MODELS:
        m = SetokimLlamaPrefill(dict(BC.LLAMA))
        m.load_state_dict(g["sd"], strict=True)
        _MODELS[(name, dt)] = m.to(device=DEV, dtype=dt).eval()
    return _MODELS[(name, dt)], g, g["x"].to(DEV), g["am"].to(DEV)


@pytest.mark.parametrize("name", list(BC.CASES))
def test_generate_with_beams_reproduces_huggingface(golden_dir, name):
    m, g, x, am = _fixture_model(golden_dir, name)
    for R, tag in ((1, "r1"), (g["n"], "rn")):
        out = m.generate(inputs_embeds=x, attention_mask=am, max_new_tokens=BC.N_NEW, eos_token_id=g["eos"], return_dict_in_generate=True,
                         beams=BeamSearch(g["n"], g["lp"], g["es"], R))
        assert torch.equal(out.sequences.cpu(), g[f"sequences_{tag}"]) and torch.equal(out.beam_indices.cpu(), g[f"beam_indices_{tag}"]), (name, R)
        rel = float(((out.sequences_scores.cpu() - g[f"scores_{tag}"]).abs() / g[f"scores_{tag}"].abs()).max())
        print(f"generate(beams) {name} R={R}: scores max rel {rel:.3e}")
        assert rel <= 1e-4, (name, R, rel)
        assert out.sequences_scores.dtype == torch.float32 and out.beam_indices.dtype == torch.int32 and out.sequences.dtype == torch.int64
        s = out.sequences_scores.view(-1, R)
        assert bool((s[:, :-1] >= s[:, 1:]).all())                                         # rows b * R + r in descending score
        plain = m.generate(inputs_embeds=x, attention_mask=am, max_new_tokens=BC.N_NEW, eos_token_id=g["eos"], beams=BeamSearch(g["n"], g["lp"], g["es"], R))
        assert torch.equal(plain, out.sequences)


def test_one_beam_without_eos_is_the_greedy_loop(golden_dir):
    m, g, x, am = _fixture_model(golden_dir, "n2_lp1_false")
    greedy = m.generate(inputs_embeds=x, attention_mask=am, max_new_tokens=BC.N_NEW)
    out = m.generate(inputs_embeds=x, attention_mask=am, max_new_tokens=BC.N_NEW, beams=BeamSearch(1), return_dict_in_generate=True)
    assert torch.equal(out.sequences, greedy)
    assert out.beam_indices.tolist() == [[b] * BC.N_NEW for b in range(BC.B)]


def test_beam_logits_match_one_teacher_forced_prefill_across_a_decode_chunk():
    """Head dim 128, grouped-query, a prompt of 120 so that the generated slots cross slot 128: each returned hypothesis, fed through ONE prefill over
    prompt + tokens, must give the ancestry-gathered logits and states under the bound the decode path holds against the prefill (1e-4).  This checks
    the cache reorder and the ancestry gather end to end, independent of HuggingFace."""
    kw, lc, seed, _, _, _, _, _ = LC.case_inputs("gqa_dh128")
    m = SetokimLlamaPrefill(kw)
    m.load_state_dict({k: v * BC.WEIGHT_SCALE for k, v in O.init_llama_weights(lc, seed=seed).items()}, strict=True)
    m = m.to(DEV).eval()
    B, T, n, n_new = 2, 120, 4, 16
    x = torch.randn(B, T, lc.hidden_size, generator=torch.Generator().manual_seed(1)).to(DEV)
    out = m.generate(inputs_embeds=x, max_new_tokens=n_new, beams=BeamSearch(n, 1.0, False, n), return_dict_in_generate=True, output_logits=True,
                     output_hidden_states=True)
    assert out.sequences.shape == (B * n, n_new) and T < CHUNK < T + n_new and int(out.beam_indices.min()) >= 0
    assert len({tuple(r) for r in out.beam_indices.tolist()}) > B                        # the hypotheses really changed rows on the way
    emb = m.model.embed_tokens.weight[out.sequences[:, :-1]]
    full = torch.cat([x.repeat_interleave(n, dim=0), emb.to(x.dtype)], dim=1)
    hidden = m.model.prefill(full, None, None, KVCache.for_model(m.model, B * n, T + n_new))[:, T - 1:]
    logits = ops.linear(hidden.reshape(-1, lc.hidden_size).contiguous(), m.lm_head.weight.detach().contiguous()).reshape(B * n, n_new, -1)
    parity.close(out.logits, logits, 1e-4, "beam logits vs teacher-forced prefill")
    parity.close(out.hidden_states, hidden, 1e-4, "beam states vs teacher-forced prefill")


def _dh128_model(dt):
    """The head-dim-128 grouped-query case of tests/llama_bwd_cases.py (every GEMM dimension a multiple of 64, as the 16-bit kernels need) with the
    fixture's weight scale, three prompts of 9 positions, the second left-padded."""
    if ("gqa_dh128", dt) not in _MODELS:
        kw, lc, seed, _, _, _, _, _ = LC.case_inputs("gqa_dh128")
        m = SetokimLlamaPrefill(kw)
        m.load_state_dict({k: v * BC.WEIGHT_SCALE for k, v in O.init_llama_weights(lc, seed=seed).items()}, strict=True)
        _MODELS[("gqa_dh128", dt)] = m.to(device=DEV, dtype=dt).eval()
    m = _MODELS[("gqa_dh128", dt)]
    x = torch.randn(BC.B, BC.T, m.model.norm.weight.shape[0], generator=torch.Generator().manual_seed(2)).to(device=DEV, dtype=dt)
    am = torch.ones(BC.B, BC.T, dtype=torch.long, device=DEV)
    am[1, :3] = 0
    return m, x, am


@pytest.mark.parametrize("dt,kv", [(torch.bfloat16, "native"), (torch.bfloat16, "fp8"), (torch.float16, "native"), (torch.float16, "fp8")])
def test_generate_with_beams_in_16_bits_and_with_the_fp8_cache(dt, kv):
    m, x, am = _dh128_model(dt)
    free = m.generate(inputs_embeds=x, attention_mask=am, max_new_tokens=BC.N_NEW, kv_cache=kv, beams=BeamSearch(3))
    eos = [int(free[0, 3]), int(free[1, 5])]                                               # ids the search itself emits: some hypotheses end early
    kw = dict(max_new_tokens=BC.N_NEW, eos_token_id=eos, return_dict_in_generate=True, kv_cache=kv, beams=BeamSearch(3, 0.6, "never", 3))
    out = m.generate(inputs_embeds=x, attention_mask=am, **kw)
    R, n_new = 3, out.sequences.shape[1]
    assert out.sequences.shape[0] == BC.B * R and 1 <= n_new <= BC.N_NEW and bool(torch.isfinite(out.sequences_scores).all())
    assert bool(torch.isin(out.sequences, torch.tensor(eos, device=DEV)).any())
    for b in range(BC.B):                                                                  # a sequence alone equals the same sequence in the batch of 3
        one = m.generate(inputs_embeds=x[b:b + 1], attention_mask=am[b:b + 1], **kw)
        k = one.sequences.shape[1]
        rows = slice(b * R, (b + 1) * R)
        assert torch.equal(one.sequences, out.sequences[rows, :k]) and bool((out.sequences[rows, k:] == eos[0]).all()), (b, dt, kv)
        assert torch.equal(one.sequences_scores, out.sequences_scores[rows])
        assert torch.equal(one.beam_indices, torch.where(out.beam_indices[rows, :k] >= 0, out.beam_indices[rows, :k] - 3 * b, -1))
    if kv == "native" and dt == torch.bfloat16:                                            # (windows extend the cache: not with the fp8 cache; the fp16 extend
                                                                                           #  kernel rounds its own way, which reorders near-tied running beams)
        chunked = m.generate(inputs_embeds=x, attention_mask=am, prefill_chunk=4, **kw)
        print(f"beams {dt} prefill_chunk=4: scores max |diff| {float((chunked.sequences_scores - out.sequences_scores).abs().max()):.3e}")
        assert torch.equal(chunked.sequences, out.sequences) and torch.equal(chunked.beam_indices, out.beam_indices)     # (the extend kernel rounds its own way: the hypotheses are equal, not the scores' last bits)
