"""MXFP4 weight-only storage on a real MI355X, through the C ABI: setok_quantize_mxfp4_rows / setok_dequantize_mxfp4_rows bit for bit against the
CPU oracle of tests/mxfp4_cases.py, setok_linear_mxfp4w against fp64 of A · W'^T with the existing `ops.linear` on W' as the yardstick, and a
quantised `SetokimLlamaPrefill` against the plain model loaded with the oracle's W' (the quantised model IS that model: no tolerance for
"quantisation error" appears anywhere).  The method of tests/test_fp8w_gpu.py.  `pytest -m gpu`."""
import pytest
import torch

import mxfp4_cases as X
import parity
import setok_oracle as O
from test_fp8w_gpu import DEV, DTYPES, NAN, TAG, _bits, _frame_untouched, _log, _window

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from setok_amd import ops
    from setok_amd.generation import KVCache, LookupDrafter
    from setok_amd.llama import SetokimLlamaPrefill

HALVES = [torch.bfloat16, torch.float16]


def _cdiv(a, b):
    return -(-a // b)


# ---- 1. quantiser and dequantiser ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,K", [(N, K) for N in (1, 17, 100) for K in (32, 160, 4096)])
def test_quantiser_and_dequantiser_equal_the_oracle_bit_for_bit(dt, N, K):
    """W, q, s and the dequantised matrix are windows of NaN / 0xAA-filled buffers.  Blocks (mxfp4_cases.special_blocks): zeros, both clamps, amax
    exactly 6 * 2^e and one ulp below 8 * 2^e, every tie in both signs, negative zero, neighbours 20 octaves apart, Gaussian rows between them."""
    W = X.quantizer_matrix(N, K, dt, seed=N + K)
    q_ref, s_ref = X.quantize_rows(W)
    if N * K >= 17 * 160:
        assert {114, 140, 127, 124} <= set(s_ref.flatten().tolist())
    wbuf, w = _window(W, 1, 8, 1, 24, NAN)
    qbuf, q = _window(torch.zeros(N, K // 2, dtype=torch.uint8), 1, 16, 2, 16, 0xAA)
    sbuf, s = _window(torch.zeros(N, K // 32, dtype=torch.uint8), 2, 3, 1, 5, 0xAA)
    ops.quantize_mxfp4_rows(w, q=q, s=s)
    assert torch.equal(q.cpu(), q_ref) and torch.equal(s.cpu(), s_ref)
    assert bool((_frame_untouched(qbuf, 1, 16, N, K // 2, nan=False) == 0xAA).all())
    assert bool((_frame_untouched(sbuf, 2, 3, N, K // 32, nan=False) == 0xAA).all())
    Wp = X.dequantize_rows(q_ref, s_ref)
    obuf, o = _window(torch.zeros(N, K, dtype=dt), 2, 7, 1, 9, NAN)                               # (an odd offset: the byte-wise path)
    ops.dequantize_mxfp4_rows(q, s, out=o)
    assert torch.equal(o.cpu().double(), Wp) and torch.equal(_bits(o.cpu()), _bits(Wp.to(dt)))
    assert _frame_untouched(obuf, 2, 7, N, K)
    dense = ops.dequantize_mxfp4_rows(q.contiguous(), s.contiguous(), dtype=dt)                   # dense, aligned rows take the packed path: the same bits
    assert torch.equal(_bits(dense.cpu()), _bits(Wp.to(dt)))
    odd_q = _window(q_ref, 0, 3, 0, 2, 0xAA)[1]                                                   # q at an odd byte offset, W aligned: byte-wise again
    assert torch.equal(_bits(ops.dequantize_mxfp4_rows(odd_q, s, dtype=dt).cpu()), _bits(Wp.to(dt)))


@pytest.mark.parametrize("dt", DTYPES)
def test_a_non_finite_weight_makes_its_block_and_only_its_block_nan(dt):
    W = X.quantizer_matrix(4, 160, dt, seed=3)[[1, 3]].clone()
    W[0, 5], W[1, 64 + 7], W[1, 128 + 9] = NAN, float("inf"), -float("inf")
    q_ref, s_ref = X.quantize_rows(W)
    q, s = ops.quantize_mxfp4_rows(W.to(DEV))
    assert torch.equal(q.cpu(), q_ref) and torch.equal(s.cpu(), s_ref)
    bad = torch.zeros(2, 5, dtype=torch.bool)
    bad[0, 0] = bad[1, 2] = bad[1, 4] = True
    assert torch.equal(s.cpu() == X.NAN_SCALE, bad) and bool((q.cpu().view(2, 5, 16)[bad] == 0).all())
    for back in (ops.dequantize_mxfp4_rows(q, s, dtype=dt).cpu(),                                 # packed and byte-wise
                 ops.dequantize_mxfp4_rows(q, s, out=_window(torch.zeros(2, 160, dtype=dt), 0, 1, 0, 1, NAN)[1]).cpu()):
        assert torch.equal(torch.isnan(back), bad.repeat_interleave(32, dim=1))
    # the GEMM sees the same matrix: a column whose row holds a NaN block is NaN, the others are not (fp32: K = 160 is allowed there)
    if dt == torch.float32:
        out = ops.linear_mxfp4w(torch.ones(3, 160, device=DEV), q, s)
        assert bool(torch.isnan(out).all())
        q2, s2 = ops.quantize_mxfp4_rows(torch.cat([W[:1], X.quantizer_matrix(4, 160, dt, seed=3)[1:2]]).to(DEV))
        out = ops.linear_mxfp4w(torch.ones(3, 160, device=DEV), q2, s2)
        assert bool(torch.isnan(out[:, 0]).all()) and bool(torch.isfinite(out[:, 1]).all())


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_scale_bytes_the_quantiser_never_emits_are_still_value_times_two_to_the_s(dt):
    """s in {100, 150}: 2^-27 and 2^23, outside [114, 140].  The values are exact in fp32 and bf16 (not in fp16, which is not tested here)."""
    g = torch.Generator().manual_seed(7)
    N, K = 48, 128
    q = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.uint8)
    s = torch.where(torch.rand(N, K // 32, generator=g) < 0.5, 100, 150).to(torch.uint8)
    Wp = X.dequantize_rows(q, s)
    assert torch.equal(Wp.to(dt).double(), Wp) and float(Wp.abs().max()) == 6.0 * 2.0 ** 23
    for back in (ops.dequantize_mxfp4_rows(q.to(DEV), s.to(DEV), dtype=dt), ops.dequantize_mxfp4_rows(_window(q, 0, 1, 0, 3, 0xAA)[1], s.to(DEV), dtype=dt)):
        assert torch.equal(_bits(back.cpu()), _bits(Wp.to(dt)))
    a = torch.randn(5, K, generator=g).to(dt)
    ref = a.double() @ Wp.t()
    ours = parity.measure(ops.linear_mxfp4w(a.to(DEV), q.to(DEV), s.to(DEV)), ref)
    yard = parity.measure(ops.linear(a.to(DEV), Wp.to(dt).to(DEV)), ref)
    _log(f"linear_mxfp4w {TAG[dt]} scale bytes 100 / 150: max-rel ours, linear, rms-rel ours, linear", ours[0], yard[0], ours[1], yard[1])
    assert ours[0] <= 1.5 * yard[0] and ours[1] <= 1.5 * yard[1], (ours, yard)


# ---- 2. + 3. the GEMM ----------------------------------------------------------------------------------------------------------------------
MS = (1, 5, 16, 17, 37, 64)
# 16-bit: one step; 3 steps, fewer than waves; 5 steps, an uneven deal; 32, an even one; 86, uneven.  fp32 adds (100, 160): K ends inside a 128-wide step.
SHAPES = [(16, 128), (100, 384), (272, 640), (1024, 4096), (48, 11008)]
_PROBLEMS = {}


def _problem(N, K, dt):
    """One seeded problem per (N, K, dt) at M = 64, shared by the tests below (rows are independent: M < 64 takes the first rows): device
    windows of NaN / 0xAA-framed buffers for a, q, s and the residual, and the fp64 reference of a · W'^T."""
    key = (N, K, dt)
    if key not in _PROBLEMS:
        a, q, s, Wp, r = X.gemm_problem(64, N, K, dt, seed=N + K)
        assert len(set(s[0].tolist())) > 1 or K == 32
        ref = a.double() @ Wp.t()
        _PROBLEMS[key] = dict(a=_window(a, 1, 16, 1, 48, NAN), q=_window(q, 1, 32, 1, 16, 0xAA), s=_window(s, 1, 3, 2, 7, 0xAA), r=_window(r, 2, 3, 1, 10, NAN),
                              w=Wp.to(dt).to(DEV), ref=ref, ref_r=ref + r.double(), a_dense=a.to(DEV), r_dense=r.to(DEV))
    return _PROBLEMS[key]


@pytest.mark.parametrize("dt,N,K", [(dt, N, K) for N, K in SHAPES for dt in DTYPES] + [(torch.float32, 100, 160)])
def test_linear_mxfp4w_against_fp64_with_linear_on_the_dequantised_weight_as_yardstick(dt, N, K):
    """For M in {1, 5, 16, 17, 37, 64}, without residual, with one, and with `out` aliasing it — every operand a window of a wider buffer — the
    kernel's max-rel and rms-rel errors against fp64 of A · W'^T are at most 1.5 x those of the existing `ops.linear` on W' (same inputs, same
    device): the project's ratio for "within the reference's drift"."""
    p = _problem(N, K, dt)
    for M in MS:
        a, q, s = p["a"][1][:M], p["q"][1], p["s"][1]
        for mode in ("plain", "residual", "aliased"):
            ref = (p["ref"] if mode == "plain" else p["ref_r"])[:M]
            res = None if mode == "plain" else p["r_dense"][:M].contiguous()
            yard = ops.linear(p["a_dense"][:M].contiguous(), p["w"], residual=res)
            if mode == "plain":
                obuf, out = _window(torch.zeros(M, N, dtype=dt), 1, 5, 2, 11, NAN)
                got = ops.linear_mxfp4w(a, q, s, out=out)
            elif mode == "residual":
                obuf, out = _window(torch.zeros(M, N, dtype=dt), 2, 3, 1, 10, NAN)             # (the residual's frame: one row stride for both)
                got = ops.linear_mxfp4w(a, q, s, residual=p["r"][1][:M], out=out)
            else:
                obuf, out = _window(p["r_dense"][:M].cpu(), 1, 5, 2, 11, NAN)
                got = ops.linear_mxfp4w(a, q, s, residual=out, out=out)
            assert got is out
            ours, theirs = parity.measure(out, ref), parity.measure(yard, ref)
            _log(f"linear_mxfp4w {TAG[dt]} M={M} N={N} K={K} {mode}: max-rel ours, linear, rms-rel ours, linear", ours[0], theirs[0], ours[1], theirs[1])
            assert bool(torch.isfinite(out).all())
            assert ours[0] <= 1.5 * theirs[0] and ours[1] <= 1.5 * theirs[1], (M, mode, ours, theirs)
            top, left = (2, 3) if mode == "residual" else (1, 5)
            assert _frame_untouched(obuf, top, left, M, N)
    for name, (top, left, fill) in dict(a=(1, 16, None), q=(1, 32, 0xAA), s=(1, 3, 0xAA)).items():      # the inputs' frames are as they were
        buf, view = p[name]
        frame = _frame_untouched(buf, top, left, *view.shape, nan=fill is None)
        assert frame if fill is None else bool((frame == fill).all())


# ---- 4. row invariance ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_a_row_alone_has_the_bits_it_has_among_37_and_64(dt):
    N, K = 272, 640
    p = _problem(N, K, dt)
    a, q, s = p["a"][1], p["q"][1], p["s"][1]
    full = {M: (ops.linear_mxfp4w(a[:M], q, s), ops.linear_mxfp4w(a[:M], q, s, residual=p["r_dense"][:M])) for M in (37, 64)}
    dense_q, dense_s = q.contiguous(), s.contiguous()
    for row in (0, 15, 16, 36):
        alone = ops.linear_mxfp4w(p["a_dense"][row:row + 1], dense_q, dense_s)                   # dense rows: other strides, same bits
        alone_r = ops.linear_mxfp4w(a[row:row + 1], q, s, residual=p["r_dense"][row:row + 1])
        for M in (37, 64):
            assert torch.equal(alone[0], full[M][0][row]) and torch.equal(alone_r[0], full[M][1][row]), (row, M)
    assert torch.equal(full[37][0], full[64][0][:37])


# ---- 4b. the band variants ------------------------------------------------------------------------------------------------------------------
def band(M, N, min_wgs):
    """NT by the rule of the header (setok_linear_mxfp4w_wgs)."""
    mt = _cdiv(M, 16)
    nt = 1 if mt == 1 else (2 if mt == 2 else 4)
    while nt > 1 and _cdiv(N, 16 * nt) < min_wgs:
        nt //= 2
    return nt


@pytest.mark.parametrize("dt", HALVES)
@pytest.mark.parametrize("N", [40, 100, 272])
def test_every_band_named_by_its_floor_has_the_bits_of_the_narrow_band(dt, N):
    """setok_linear_mxfp4w_wgs with min_wgs = ceil(N / (16 NT)) takes NT (where the row tiles allow it), min_wgs = ceil(N / 16) takes NT = 1: all
    nine (row tiles, NT) variants, without and with an aliased residual, inside a NaN frame, `torch.equal` to NT = 1 and to the public call.
    N = 40 and 100 end inside a band; K = 2176 is 17 steps: every variant's loop (4, 16 or 32 steps per round of the workgroup) runs a partly filled
    round, the 4- and 16-step ones more than one."""
    K = 2176
    p = _problem(N, K, dt)
    seen = set()
    for M in (1, 17, 33, 48, 64):
        a, q, s = p["a"][1][:M], p["q"][1], p["s"][1]
        for res in (False, True):
            r = p["r_dense"][:M] if res else None
            narrow = ops.linear_mxfp4w(a, q, s, residual=r, min_wgs=_cdiv(N, 16))
            assert band(M, N, _cdiv(N, 16)) == 1 and torch.equal(narrow, ops.linear_mxfp4w(a, q, s, residual=r))
            assert parity.measure(narrow, (p["ref_r"] if res else p["ref"])[:M])[0] < 1e-2
            for want in (1, 2, 4):
                floor = _cdiv(N, 16 * want)
                nt = band(M, N, floor)
                assert nt == min(want, (1, 1, 2, 4, 4)[_cdiv(M, 16)])
                seen.add((_cdiv(M, 16), nt))
                obuf, out = _window(r.cpu() if res else torch.zeros(M, N, dtype=dt), 2, 3, 1, 10, NAN)
                ops.linear_mxfp4w(a, q, s, residual=out if res else None, out=out, min_wgs=floor)
                assert _frame_untouched(obuf, 2, 3, M, N) and torch.equal(out, narrow), (M, res, want)
    assert seen == {(1, 1), (2, 1), (2, 2), (3, 1), (3, 2), (3, 4), (4, 1), (4, 2), (4, 4)}


def test_more_than_64_rows_dequantise_into_the_callers_scratch():
    dt, N, K = torch.bfloat16, 272, 640
    p = _problem(N, K, dt)
    a = torch.cat([p["a_dense"], p["a_dense"].flip(0)], 0)                                       # 128 rows
    with pytest.raises(ValueError, match="scratch"):
        ops.linear_mxfp4w(a, p["q"][1], p["s"][1])
    scratch = torch.empty(N * K + 7, dtype=dt, device=DEV)
    got = ops.linear_mxfp4w(a, p["q"][1], p["s"][1], scratch=scratch)
    assert torch.equal(got, ops.linear(a, p["w"]))


# ---- 5. the model -----------------------------------------------------------------------------------------------------------------------------
N_NEW = 8
MODEL_CASES = [("mx_tiny_left", torch.float32)] + [(n, dt) for n in ("dh128_left", "gqa_dh128") for dt in DTYPES]
# case -> seed of the weights where the case's own seed leaves more than 1/8 of the steps with a top-2 margin below 1e-3 on the CPU oracle
# (O.llama_forward on mxfp4_cases.quantized_state_dict, greedy, 8 steps): mx_tiny_left 1 of 24, dh128_left 0 of 16, gqa_dh128 0 of 16 — none needed.
SEEDS = {}
_MODELS = {}


def _model(name, dt, kind):
    """kind "Q": built from O.init_llama_weights, cast to `dt` on the device, then quantised.  kind "P": the plain path loaded with the oracle's W'
    of the weights as a `dt` model holds them.  kind "P32": that same state dict in an fp32 model — the reference of the 16-bit drift."""
    kw, lc, seed, x, am, pos = X.case_inputs(name)
    key = (name, dt, kind)
    if key not in _MODELS:
        sd = O.init_llama_weights(lc, seed=SEEDS.get(name, seed))
        m = SetokimLlamaPrefill(kw)
        if kind == "Q":
            m.load_state_dict(sd, strict=True)
            m = m.to(device=DEV, dtype=dt).eval()
            m.quantize_mxfp4_()
        else:
            m.load_state_dict(X.quantized_state_dict(sd, dt), strict=True)
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


def _generate(m, x, am, pos, **kw):
    return m.generate(inputs_embeds=x, attention_mask=am, position_ids=pos, max_new_tokens=N_NEW, return_dict_in_generate=True, output_logits=True, **kw)


@pytest.mark.parametrize("name,dt", MODEL_CASES)
def test_quantised_model_is_the_plain_model_on_the_dequantised_weights(name, dt):
    q_m, x, am, pos = _model(name, dt, "Q")
    p32, _, _, _ = _model(name, dt, "P32")
    assert q_m.weight_format == "mxfp4_e2m1" and q_m.model.weight_format == "mxfp4_e2m1" and p32.weight_format == "native"
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
        parity.close(lq, ref, 1e-4, f"{name} fp32: mxfp4 model's teacher-forced logits against the plain model on W'")
        assert torch.equal(lq[0], ref[0])                  # P's prefill is the quantised model's bit for bit: the same kernels on the same (dequantised) weights
        top2 = ref.topk(2, dim=-1).values
        margin = ((top2[..., 0] - top2[..., 1]) / ref.abs().amax(dim=-1)).cpu()
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


def _prefilled(m, xs, T):
    cache = KVCache.for_model(m.model, xs.shape[0], T + 2)
    m.model.prefill(xs, None, None, cache)
    return cache


@pytest.mark.parametrize("name,dt", [("mx_tiny_left", torch.float32), ("dh128_left", torch.bfloat16)])
def test_a_decode_step_of_65_sequences_dequantises_and_equals_the_plain_model(name, dt):
    """B = 65 is past the streaming kernel: every GEMM of the step dequantises its matrix into the model's one scratch buffer and runs `linear` —
    the plain model's calls on the plain model's weights, so the states are `torch.equal`; one more step too."""
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


def test_a_quantised_sequence_alone_generates_what_it_generates_in_the_batch():
    m, x, am, pos = _model("dh128_left", torch.bfloat16, "Q")
    x = x.to(torch.bfloat16)
    kw = dict(max_new_tokens=12, return_dict_in_generate=True, output_logits=True)
    full = m.generate(inputs_embeds=x, attention_mask=am, position_ids=pos, **kw)
    for b in range(x.shape[0]):
        one = m.generate(inputs_embeds=x[b:b + 1], attention_mask=am[b:b + 1], position_ids=pos[b:b + 1], **kw)
        assert torch.equal(one.sequences[0], full.sequences[b]) and torch.equal(one.logits[0], full.logits[b])


@pytest.mark.parametrize("Tn", [8, 40])                                    # B * Tn = 16 (the streaming GEMM) and 80 (the dequantise scratch)
def test_extend_on_mxfp4_weights_equals_the_decode_steps_token_by_token(Tn):
    """The last Tn columns of the left-padded prompt (all attended) appended by ONE extend against Tn decode steps on the same quantised model,
    within the fp32 1e-4 bound tests/test_extend_gpu.py holds extend to on fp8 weights."""
    m, x, am, pos = _model("dh128_left", torch.float32, "Q")
    B, T, D = x.shape
    assert (B * Tn <= ops.MXFP4W_MAX_M) == (Tn == 8) and bool(am[:, T - Tn:].all())
    caches = [KVCache.for_model(m.model, B, T) for _ in range(2)]
    for c in caches:
        m.model.prefill(x[:, :T - Tn], am[:, :T - Tn], pos[:, :T - Tn], c)
    hid = m.model.extend(x[:, T - Tn:], caches[0], am[:, T - Tn:])
    steps = torch.stack([m.model.decode_step(x[:, T - Tn + j].contiguous(), caches[1]) for j in range(Tn)], dim=1)
    assert caches[0].len == T and caches[1].len == T and torch.equal(caches[0].next_pos, caches[1].next_pos)
    parity.close(hid, steps, 1e-4, f"mxfp4 weights, extend of {Tn} rows against {Tn} decode steps")


def test_a_draft_and_an_fp8_kv_cache_keep_their_invariants_on_mxfp4_weights():
    from test_fp8kv_gpu import _check_loop
    m, x, am, pos = _model("dh128_left", torch.float32, "Q")
    g = dict(inputs_embeds=x, attention_mask=am, position_ids=pos, max_new_tokens=12)
    assert torch.equal(m.generate(draft=LookupDrafter(3), **g), m.generate(**g))                  # speculation changes no token
    mb, xb, amb, posb = _model("dh128_left", torch.bfloat16, "Q")
    out = _check_loop(mb, xb.to(torch.bfloat16), amb, posb)                                       # kv_cache="fp8": the loop is its own teacher-forced run
    native = _generate(mb, xb.to(torch.bfloat16), amb, posb)
    assert torch.equal(native.logits[:, 0], out.logits[:, 0])                                     # step 0 is the prefill, which the cache's format does not touch


# ---- 6. the contract ----------------------------------------------------------------------------------------------------------------------------
def _fresh(name, dt):
    kw, lc, seed, x, am, pos = X.case_inputs(name)
    m = SetokimLlamaPrefill(kw)
    m.load_state_dict(O.init_llama_weights(lc, seed=seed), strict=True)
    return m.to(device=DEV, dtype=dt).eval(), x.to(DEV).to(dt), am.to(DEV), pos.to(DEV)


MATS = ("wqkv", "wo", "wgu", "wd")


def test_storage_and_refusals_of_a_quantised_model():
    name, dt = "gqa_dh128", torch.bfloat16
    m, x, am, pos = _fresh(name, dt)
    lins = [l for l in m.model.layers.modules() if isinstance(l, torch.nn.Linear)]
    shapes = [tuple(l.weight.shape) for l in lins]
    assert m.weight_format == "native"
    assert m.quantize_mxfp4_() is m and m.weight_format == "mxfp4_e2m1" and m.model._quant["fmt"].tag == "mxfp4"
    assert all(l.weight.untyped_storage().nbytes() == 0 for l in lins)                            # the masters are gone ...
    held = sum(q.numel() * q.element_size() + s.numel() * s.element_size() for L in m.model._quant["layers"] for q, s in (L[k] for k in MATS))
    assert held == sum(n * k // 2 + n * k // 32 for n, k in shapes)                               # ... N K / 2 + N K / 32 bytes per matrix remain
    assert all(q.dtype == torch.uint8 and s.dtype == torch.uint8 for L in m.model._quant["layers"] for q, s in (L[k] for k in MATS))
    assert m.lm_head.weight.numel() and m.model.embed_tokens.weight.numel()                       # embed_tokens and lm_head stay
    for call in (m.state_dict, m.model.state_dict, m.quantize_mxfp4_, m.quantize_fp8_, m.model.quantize_fp8_,
                 lambda: m.model.add_lora_(64, 128.0), lambda: m.to(torch.float16)(inputs_embeds=x.half(), attention_mask=am, position_ids=pos)):
        with pytest.raises(NotImplementedError, match="mxfp4"):
            call()
    m.to(dt)
    with torch.enable_grad():
        xg = x.clone().requires_grad_(True)
        with pytest.raises(NotImplementedError, match="mxfp4"):
            m(inputs_embeds=xg, attention_mask=am, position_ids=pos)
        with pytest.raises(NotImplementedError, match="mxfp4"):
            m.model(xg, am, pos)
    assert m(inputs_embeds=x, attention_mask=am, position_ids=pos)[0].shape[:2] == x.shape[:2]    # inference still runs
    # the reverse order, and a stack with adapters
    f8, _, _, _ = _fresh("dh128_left", dt)
    f8.quantize_fp8_()
    with pytest.raises(NotImplementedError, match="mxfp4"):
        f8.quantize_mxfp4_()
    assert f8.weight_format == "fp8_e4m3" and f8.model._quant["fmt"].tag == "fp8"
    lo, _, _, _ = _fresh("dh128_left", dt)
    lo.model.add_lora_(64, 128.0)
    with pytest.raises(NotImplementedError, match=r"quantize_mxfp4_.*merge_lora_\(\)"):
        lo.quantize_mxfp4_()
    assert lo.weight_format == "native"
    # a size off the K granule: refused by the matrix's name before anything is freed (intermediate 176 holds no whole number of blocks)
    odd, _, _, _ = _fresh("tiny_left", torch.float32)
    with pytest.raises(ValueError, match=r"mlp\.down_proj.*176"):
        odd.quantize_mxfp4_()
    assert odd.weight_format == "native" and all(p.numel() for p in odd.parameters())
    # free_master=False keeps the masters for state_dict(), and the copy cannot follow an update of them
    keep, kx, kam, kpos = _fresh("mx_tiny_left", torch.float32)
    keep.quantize_mxfp4_(free_master=False)
    assert len(keep.state_dict()) == len(O.init_llama_weights(X.case_inputs("mx_tiny_left")[1], seed=1))
    keep(inputs_embeds=kx, attention_mask=kam, position_ids=kpos)
    keep.model.layers[0].self_attn.q_proj.weight.mul_(1.5)
    with pytest.raises(NotImplementedError, match="mxfp4"):
        keep(inputs_embeds=kx, attention_mask=kam, position_ids=kpos)


@pytest.mark.parametrize("kind", ["native", "fp8"])
def test_other_models_never_reach_the_mxfp4_entry_points(monkeypatch, kind):
    m, x, am, pos = _fresh("dh128_left", torch.bfloat16)
    if kind == "fp8":
        m.quantize_fp8_()
    B, T = x.shape[:2]

    def step():
        cache = KVCache.for_model(m.model, B, T + 2)
        h = m.model.prefill(x, am, pos, cache)
        return m.model.decode_step(h[:, -1].contiguous(), cache)

    plain = step()

    def never(*a, **k):
        raise AssertionError(f"a {kind} model called an mxfp4 entry point")

    for fn in ("linear_mxfp4w", "quantize_mxfp4_rows", "dequantize_mxfp4_rows"):
        monkeypatch.setattr(ops, fn, never)
    assert torch.equal(step(), plain)
