"""FP8 weight-only storage on a real MI355X, through the C ABI: setok_quantize_fp8_rows / setok_dequantize_fp8_rows bit for bit against the CPU
oracle of tests/fp8_cases.py, setok_linear_fp8w against fp64 of A · W'^T with the existing `ops.linear` on W' as the yardstick, and a quantised
`SetokimLlamaPrefill` against the plain model loaded with the oracle's W' (the quantised model IS that model: no tolerance for "quantisation
error" appears anywhere).  `pytest -m gpu`."""
import os

import pytest
import torch

import fp8_cases as F
import llama_bwd_cases as C
import parity
import setok_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from setok_amd import ops
    from setok_amd.generation import KVCache
    from setok_amd.llama import SetokimLlamaPrefill

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
TAG = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}
NAN = float("nan")


def _log(label, *nums):
    path = os.environ.get("SETOK_PARITY_LOG")
    if path:
        test = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]
        with open(path, "a") as f:
            f.write(f"{test}\t{label}\t" + "\t".join(f"{n:.3e}" for n in nums) + "\n")
    print(label, *[f"{n:.3e}" for n in nums])


def _window(t, top, left, bottom, right, fill):
    """(buffer, view): `t` on the device as a window of a buffer that is wider and taller, the frame filled with `fill`."""
    R, Cc = t.shape
    buf = torch.full((R + top + bottom, Cc + left + right), fill, dtype=t.dtype, device=DEV)
    view = buf[top:top + R, left:left + Cc]
    view.copy_(t)
    return buf, view


def _frame_untouched(buf, top, left, R, Cc, nan=True):
    m = torch.ones_like(buf, dtype=torch.bool)
    m[top:top + R, left:left + Cc] = False
    frame = buf[m]
    return bool(torch.isnan(frame).all()) if nan else frame


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---- 1. quantiser and dequantiser ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,K", [(N, K) for N in (1, 17, 100) for K in (16, 176, 4096)])
def test_quantiser_and_dequantiser_equal_the_oracle_bit_for_bit(dt, N, K):
    """W is a window (ldw > K) of a NaN-filled buffer; q and the dequantised matrix are windows too.  Rows: all zeros, amax 1e-8 and 1e-6 (clamp at
    -15), amax 1e5 (clamp at 7, saturating), amax exactly 448 * 2^-6 and one ulp above, rounding ties, fp8-subnormal results, negative zero."""
    W = F.quantizer_matrix(N, K, dt, seed=N + K)
    q_ref, e_ref = F.quantize_rows(W)
    if N >= 17:
        assert {-15, 7, 0, -6, -5} <= set(e_ref.tolist())
    wbuf, w = _window(W, 1, 8, 1, 24, NAN)
    qbuf, q = _window(torch.zeros(N, K, dtype=torch.uint8), 1, 16, 2, 16, 0xAA)
    e = torch.full((N + 2,), 99, dtype=torch.int8, device=DEV)
    ops.quantize_fp8_rows(w, q=q, e=e[1:N + 1])
    assert torch.equal(q.cpu(), q_ref) and torch.equal(e[1:N + 1].cpu(), e_ref)
    assert e[0] == 99 and e[N + 1] == 99 and bool((_frame_untouched(qbuf, 1, 16, N, K, nan=False) == 0xAA).all())
    Wp = F.dequantize_rows(q_ref, e_ref)
    obuf, o = _window(torch.zeros(N, K, dtype=dt), 2, 7, 1, 9, NAN)                               # (an odd offset: the byte-wise path)
    ops.dequantize_fp8_rows(q, e[1:N + 1].contiguous(), out=o)
    assert torch.equal(o.cpu().double(), Wp) and torch.equal(_bits(o.cpu()), _bits(Wp.to(dt)))
    assert _frame_untouched(obuf, 2, 7, N, K)
    dense = ops.dequantize_fp8_rows(q.contiguous(), e[1:N + 1].contiguous(), dtype=dt)            # dense, aligned rows take the four-byte path: the same bits
    assert torch.equal(_bits(dense.cpu()), _bits(Wp.to(dt)))


@pytest.mark.parametrize("dt", DTYPES)
def test_quantiser_keeps_a_non_finite_weight_visible(dt):
    W = F.quantizer_matrix(4, 64, dt, seed=3)[[1, 3]].clone()
    W[0, 5], W[1, 7], W[1, 9] = NAN, float("inf"), -float("inf")
    q_ref, e_ref = F.quantize_rows(W)
    q, e = ops.quantize_fp8_rows(W.to(DEV))
    assert torch.equal(q.cpu(), q_ref) and torch.equal(e.cpu(), e_ref)
    assert int(q[0, 5]) == F.NAN_CODE and int(q[1, 7]) == F.NAN_CODE and int(q[1, 9]) == F.NAN_CODE
    back = ops.dequantize_fp8_rows(q, e, dtype=dt).cpu()
    assert torch.equal(torch.isnan(back), ~torch.isfinite(W))


# ---- 2. + 3. the GEMM ----------------------------------------------------------------------------------------------------------------------
MS = (1, 5, 16, 17, 37, 64)
SHAPES = [(16, 64), (100, 176), (272, 256), (1024, 4096), (48, 11008)]
_PROBLEMS = {}


def _problem(N, K, dt):
    """One seeded problem per (N, K, dt) at M = 64, shared by the tests below (rows are independent: M < 64 takes the first rows):
    device windows of NaN-framed buffers for a, q and the residual, and the fp64 reference of a · W'^T."""
    key = (N, K, dt)
    if key not in _PROBLEMS:
        a, q, e, Wp, r = F.gemm_problem(64, N, K, dt, seed=N + K)
        ref = a.double() @ Wp.t()
        _PROBLEMS[key] = dict(a=_window(a, 1, 16, 1, 48, NAN), q=_window(q, 1, 32, 1, 16, F.NAN_CODE), e=e.to(DEV), r=_window(r, 2, 3, 1, 10, NAN),
                              w=Wp.to(dt).to(DEV), ref=ref, ref_r=ref + r.double(), a_dense=a.to(DEV), r_dense=r.to(DEV))
    return _PROBLEMS[key]


@pytest.mark.parametrize("dt,N,K", [(dt, N, K) for N, K in SHAPES for dt in DTYPES if K % 64 == 0 or dt == torch.float32])      # (K = 176: fp32 only)
def test_linear_fp8w_against_fp64_with_linear_on_the_dequantised_weight_as_yardstick(dt, N, K):
    """For M in {1, 5, 16, 17, 37, 64}, without residual, with one, and with `out` aliasing it — every operand a window of a wider buffer —
    the kernel's max-rel and rms-rel errors against fp64 of A · W'^T are at most 1.5 x those of the existing `ops.linear` on W' (same inputs,
    same device): the project's ratio for "within the reference's drift"."""
    p = _problem(N, K, dt)
    for M in MS:
        a, q = p["a"][1][:M], p["q"][1]
        for mode in ("plain", "residual", "aliased"):
            ref = (p["ref"] if mode == "plain" else p["ref_r"])[:M]
            res = None if mode == "plain" else p["r_dense"][:M].contiguous()
            yard = ops.linear(p["a_dense"][:M].contiguous(), p["w"], residual=res)
            if mode == "plain":
                obuf, out = _window(torch.zeros(M, N, dtype=dt), 1, 5, 2, 11, NAN)
                got = ops.linear_fp8w(a, q, p["e"], out=out)
            elif mode == "residual":
                obuf, out = _window(torch.zeros(M, N, dtype=dt), 2, 3, 1, 10, NAN)             # (the residual's frame: one row stride for both)
                got = ops.linear_fp8w(a, q, p["e"], residual=p["r"][1][:M], out=out)
            else:
                obuf, out = _window(p["r_dense"][:M].cpu(), 1, 5, 2, 11, NAN)
                got = ops.linear_fp8w(a, q, p["e"], residual=out, out=out)
            assert got is out
            ours, theirs = parity.measure(out, ref), parity.measure(yard, ref)
            _log(f"linear_fp8w {TAG[dt]} M={M} N={N} K={K} {mode}: max-rel ours, linear, rms-rel ours, linear", ours[0], theirs[0], ours[1], theirs[1])
            assert bool(torch.isfinite(out).all())
            assert ours[0] <= 1.5 * theirs[0] and ours[1] <= 1.5 * theirs[1], (M, mode, ours, theirs)
            top, left = (2, 3) if mode == "residual" else (1, 5)
            assert _frame_untouched(obuf, top, left, M, N)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M", [1, 17, 64])
def test_linear_fp8w_touches_nothing_outside_its_operands(dt, M):
    """C inside a NaN-filled buffer wider and taller than (M, N); A and q likewise framed with NaN (q: the NaN code): every element outside
    [0, M) x [0, N) is still NaN, every element inside is finite.  N = 100 ends inside a 16-column band, K ends inside a 64-wide step in fp32."""
    N, K = (100, 176) if dt == torch.float32 else (100, 192)
    p = _problem(N, K, dt)
    for res in (False, True):
        obuf, out = _window(torch.zeros(M, N, dtype=dt), 2, 3, 1, 10, NAN)
        ops.linear_fp8w(p["a"][1][:M], p["q"][1], p["e"], residual=p["r"][1][:M] if res else None, out=out)
        assert bool(torch.isfinite(out).all()) and _frame_untouched(obuf, 2, 3, M, N)
        assert parity.measure(out, (p["ref_r"] if res else p["ref"])[:M])[0] < (1e-5 if dt == torch.float32 else 1e-2)


# ---- 4. row invariance ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_a_row_alone_has_the_bits_it_has_among_37_and_64(dt):
    N, K = 272, 256
    p = _problem(N, K, dt)
    a, q, e = p["a"][1], p["q"][1], p["e"]
    full = {M: (ops.linear_fp8w(a[:M], q, e), ops.linear_fp8w(a[:M], q, e, residual=p["r_dense"][:M])) for M in (37, 64)}
    dense_q = q.contiguous()
    for row in (0, 15, 16, 36):
        alone = ops.linear_fp8w(p["a_dense"][row:row + 1], dense_q, e)                           # dense rows: other strides, same bits
        alone_r = ops.linear_fp8w(a[row:row + 1], q, e, residual=p["r_dense"][row:row + 1])
        for M in (37, 64):
            assert torch.equal(alone[0], full[M][0][row]) and torch.equal(alone_r[0], full[M][1][row]), (row, M)
    assert torch.equal(full[37][0], full[64][0][:37])


def test_more_than_64_rows_dequantise_into_the_callers_scratch():
    dt, N, K = torch.bfloat16, 272, 256
    p = _problem(N, K, dt)
    a = torch.cat([p["a_dense"], p["a_dense"].flip(0)], 0)                                       # 128 rows
    with pytest.raises(ValueError, match="scratch"):
        ops.linear_fp8w(a, p["q"][1], p["e"])
    scratch = torch.empty(N * K + 7, dtype=dt, device=DEV)
    got = ops.linear_fp8w(a, p["q"][1], p["e"], scratch=scratch)
    assert torch.equal(got, ops.linear(a, p["w"]))


# ---- 5. the model -----------------------------------------------------------------------------------------------------------------------------
N_NEW = 8
MODEL_CASES = [("tiny_left", torch.float32), ("gqa_tiny_left", torch.float32)] + [(n, dt) for n in ("dh128_left", "gqa_dh128") for dt in DTYPES]
SEEDS = {}                       # case -> seed of the weights where the case's own seed (tests/llama_bwd_cases.py) leaves too many narrow margins
_MODELS = {}


def _model(name, dt, kind):
    """kind "Q": built from O.init_llama_weights, cast to `dt` on the device, then quantised.  kind "P": the plain path loaded with the oracle's W'
    of the weights as a `dt` model holds them.  kind "P32": that same state dict in an fp32 model — the reference of the 16-bit drift."""
    kw, lc, seed, x, am, pos, _, _ = C.case_inputs(name)
    key = (name, dt, kind)
    if key not in _MODELS:
        sd = O.init_llama_weights(lc, seed=SEEDS.get(name, seed))
        m = SetokimLlamaPrefill(kw)
        if kind == "Q":
            m.load_state_dict(sd, strict=True)
            m = m.to(device=DEV, dtype=dt).eval()
            m.quantize_fp8_()
        else:
            m.load_state_dict(F.quantized_state_dict(sd, dt), strict=True)
            m = m.to(device=DEV, dtype=torch.float32 if kind == "P32" else dt).eval()
        _MODELS[key] = m
    return _MODELS[key], x.to(DEV), am.to(DEV), pos.to(DEV)


def _teacher_forced(m, x, am, pos, tokens):
    """Prefill + decode_step feeding `tokens` (n, B): logits (n, B, V) — the logits that predict token j."""
    n, B = tokens.shape
    T = x.shape[1]
    cache = KVCache.for_model(m.model, B, T + n)
    hidden = m.model.prefill(x, am, pos, cache)
    last = (am.bool() * torch.arange(T, device=x.device)[None]).max(dim=1).values
    h = hidden[torch.arange(B, device=x.device), last].contiguous()
    w_lm, w_e = m.lm_head.weight.detach().contiguous(), m.model.embed_tokens.weight.detach()
    lgs = []
    for j in range(n):
        lgs.append(ops.linear(h, w_lm))
        if j + 1 < n:
            h = m.model.decode_step(w_e[tokens[j].to(x.device)], cache)
    return torch.stack(lgs)


def _generate(m, x, am, pos):
    return m.generate(inputs_embeds=x, attention_mask=am, position_ids=pos, max_new_tokens=N_NEW, return_dict_in_generate=True, output_logits=True)


@pytest.mark.parametrize("name,dt", MODEL_CASES)
def test_quantised_model_is_the_plain_model_on_the_dequantised_weights(name, dt):
    q_m, x, am, pos = _model(name, dt, "Q")
    p32, _, _, _ = _model(name, dt, "P32")
    assert q_m.weight_format == "fp8_e4m3" and q_m.model.weight_format == "fp8_e4m3" and p32.weight_format == "native"
    B, T = x.shape[:2]
    xq = x.to(dt)
    cache = KVCache.for_model(q_m.model, B, T + N_NEW)
    assert torch.equal(q_m.model.prefill(xq, am, pos, cache), q_m.model._forward(xq, am, pos))     # the cached prefill keeps _forward's bits
    ref_out = _generate(p32, x, am, pos)
    tokens = ref_out.sequences.t().contiguous()                                                   # (n, B): P's own greedy tokens in fp32
    ref = _teacher_forced(p32, x, am, pos, tokens)
    assert torch.equal(ref, ref_out.logits.transpose(0, 1))
    lq = _teacher_forced(q_m, xq, am, pos, tokens)
    if dt == torch.float32:
        parity.close(lq, ref, 1e-4, f"{name} fp32: quantised model's teacher-forced logits against the plain model on W'")
        # P's prefill is the quantised model's bit for bit: the same kernels on the same (dequantised) weights
        assert torch.equal(lq[0], ref[0])
        top2 = ref.topk(2, dim=-1).values
        margin = ((top2[..., 0] - top2[..., 1]) / ref.abs().amax(dim=-1)).cpu()                   # the fixtures' rule (make_golden_generate.py)
        narrow = margin < 1e-3
        _log(f"{name} fp32: min top-2 margin of P, steps excluded, steps", float(margin.min()), float(narrow.sum()), float(narrow.numel()))
        assert int(narrow.sum()) * 8 <= narrow.numel(), "too many narrow margins: declare another seed for this case in SEEDS"
        got = _generate(q_m, xq, am, pos).sequences.t().cpu()
        for b in range(B):
            for j in range(N_NEW):
                if not narrow[j, b]:
                    assert int(got[j, b]) == int(tokens[j, b]), (name, j, b)
                elif int(got[j, b]) != int(tokens[j, b]):
                    break                                                                         # a coin-flip step went the other way: the rest differs by right
    else:
        p_dt, _, _, _ = _model(name, dt, "P")
        lp = _teacher_forced(p_dt, xq, am, pos, tokens)
        ours, plain = parity.measure(lq.float(), ref), parity.measure(lp.float(), ref)
        _log(f"{name} {TAG[dt]} teacher-forced logits against P in fp32: Q max-rel, P max-rel, ratio, Q rms-rel, P rms-rel, ratio",
             ours[0], plain[0], ours[0] / plain[0], ours[1], plain[1], ours[1] / plain[1])
        assert ours[0] <= 1.5 * plain[0] and ours[1] <= 1.5 * plain[1], (ours, plain)
    out = _generate(q_m, xq, am, pos)                                                             # the loop's logits are its own teacher-forced logits
    assert torch.equal(_teacher_forced(q_m, xq, am, pos, out.sequences.t().contiguous()), out.logits.transpose(0, 1))


@pytest.mark.parametrize("name,dt", [("tiny_left", torch.float32), ("dh128_left", torch.bfloat16)])
def test_a_decode_step_of_65_sequences_dequantises_and_equals_the_plain_model(name, dt):
    """B = 65 is past the streaming kernel: every GEMM of the step dequantises its matrix into the model's one scratch buffer (reused four times
    per layer) and runs `linear` — the plain model's calls on the plain model's weights, so the states are `torch.equal`; one more step too."""
    q_m, x, am, pos = _model(name, dt, "Q")
    p_m, _, _, _ = _model(name, dt, "P32" if dt == torch.float32 else "P")
    B, T, D = 65, 6, x.shape[2]
    g = torch.Generator().manual_seed(65)
    xs = torch.randn(B, T, D, generator=g).to(dt).to(DEV)
    steps = [torch.randn(B, D, generator=g).to(dt).to(DEV) for _ in range(2)]
    outs = []
    for m in (q_m, p_m):
        cache = KVCache.for_model(m.model, B, T + 2)
        hs = [m.model.prefill(xs, None, None, cache)[:, -1]]
        hs += [m.model.decode_step(e, cache) for e in steps]
        outs.append(torch.stack(hs))
    assert bool(torch.isfinite(outs[0]).all()) and torch.equal(outs[0], outs[1])
    small = q_m.model.decode_step(steps[0][:3], _prefilled(q_m, xs[:3], T))                         # the same rows through the streaming kernel: the same function
    assert parity.measure(small, outs[0][1][:3])[0] < (1e-5 if dt == torch.float32 else 3e-2)


def _prefilled(m, xs, T):
    cache = KVCache.for_model(m.model, xs.shape[0], T + 2)
    m.model.prefill(xs, None, None, cache)
    return cache


# ---- 6. batch independence --------------------------------------------------------------------------------------------------------------------
def test_a_quantised_sequence_alone_generates_what_it_generates_in_the_batch():
    m, x, am, pos = _model("dh128_left", torch.bfloat16, "Q")
    x = x.to(torch.bfloat16)
    kw = dict(max_new_tokens=12, return_dict_in_generate=True, output_logits=True)
    full = m.generate(inputs_embeds=x, attention_mask=am, position_ids=pos, **kw)
    for b in range(x.shape[0]):
        one = m.generate(inputs_embeds=x[b:b + 1], attention_mask=am[b:b + 1], position_ids=pos[b:b + 1], **kw)
        assert torch.equal(one.sequences[0], full.sequences[b]) and torch.equal(one.logits[0], full.logits[b])


# ---- 7. the contract ----------------------------------------------------------------------------------------------------------------------------
def _fresh(name, dt):
    kw, lc, seed, x, am, pos, _, _ = C.case_inputs(name)
    m = SetokimLlamaPrefill(kw)
    m.load_state_dict(O.init_llama_weights(lc, seed=seed), strict=True)
    return m.to(device=DEV, dtype=dt).eval(), x.to(DEV).to(dt), am.to(DEV), pos.to(DEV)


def test_storage_and_refusals_of_a_quantised_model():
    name, dt = "gqa_dh128", torch.bfloat16
    m, x, am, pos = _fresh(name, dt)
    lins = [l for l in m.model.layers.modules() if isinstance(l, torch.nn.Linear)]
    shapes = [tuple(l.weight.shape) for l in lins]
    assert m.weight_format == "native"
    assert m.quantize_fp8_() is m and m.weight_format == "fp8_e4m3"
    assert all(l.weight.untyped_storage().nbytes() == 0 for l in lins)                            # the masters are gone ...
    held = sum(q.numel() * q.element_size() + e.numel() * e.element_size() for L in m.model._quant["layers"] for q, e in (L[k] for k in ("wqkv", "wo", "wgu", "wd")))
    assert held == sum(n * k + n for n, k in shapes)                                              # ... N * K + N bytes per matrix remain
    assert all(q.dtype == torch.uint8 and e.dtype == torch.int8 for L in m.model._quant["layers"] for q, e in (L[k] for k in ("wqkv", "wo", "wgu", "wd")))
    assert m.lm_head.weight.numel() and m.model.embed_tokens.weight.numel()                       # embed_tokens and lm_head stay
    with pytest.raises(NotImplementedError, match="fp8"):
        m.state_dict()
    with pytest.raises(NotImplementedError, match="fp8"):
        m.model.state_dict()
    with pytest.raises(NotImplementedError, match="fp8"):
        m.quantize_fp8_()
    with torch.enable_grad():
        xg = x.clone().requires_grad_(True)
        with pytest.raises(NotImplementedError, match="fp8"):
            m(inputs_embeds=xg, attention_mask=am, position_ids=pos)
        with pytest.raises(NotImplementedError, match="fp8"):
            m.model(xg, am, pos)
    assert m(inputs_embeds=x, attention_mask=am, position_ids=pos)[0].shape[:2] == x.shape[:2]    # inference still runs
    keep, _, _, _ = _fresh("tiny_left", torch.float32)
    keep.quantize_fp8_(free_master=False)
    assert len(keep.state_dict()) == len(O.init_llama_weights(C.case_inputs("tiny_left")[1], seed=1))   # the masters stayed: saving them works
    kx, kam, kpos = (t.to(DEV) for t in C.case_inputs("tiny_left")[3:6])
    keep(inputs_embeds=kx, attention_mask=kam, position_ids=kpos)
    keep.model.layers[0].self_attn.q_proj.weight.mul_(1.5)                                        # ... but the fp8 copy cannot follow an update of them
    with pytest.raises(NotImplementedError, match="fp8"):
        keep(inputs_embeds=kx, attention_mask=kam, position_ids=kpos)


def test_an_unquantised_model_never_reaches_the_fp8_entry_points(monkeypatch):
    m, x, am, pos = _fresh("dh128_left", torch.bfloat16)
    B, T = x.shape[:2]

    def step():
        cache = KVCache.for_model(m.model, B, T + 2)
        h = m.model.prefill(x, am, pos, cache)
        return m.model.decode_step(h[:, -1].contiguous(), cache)

    plain = step()

    def never(*a, **k):
        raise AssertionError("an unquantised model called an fp8 entry point")

    for fn in ("linear_fp8w", "quantize_fp8_rows", "dequantize_fp8_rows"):
        monkeypatch.setattr(ops, fn, never)
    assert torch.equal(step(), plain)
