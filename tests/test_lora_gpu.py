"""LoRA fine-tuning of the Llama stack on a real MI355X: the skinny GEMM against float64, at strides and for bit invariance; the adapted model's
loss and gradients against HuggingFace's autograd with the LoRA rule wrapped around its Linears (tests/golden/lora.npz, written by
tests/golden/make_golden_lora.py); fresh adapters, a target subset, dropout, a short training run, merging and the refusals.  `pytest -m gpu`."""
import os

import numpy as np
import pytest
import torch

import golden_io
import llama_bwd_cases as C
import lora_cases as LC
import parity
import setok_oracle as O

pytestmark = pytest.mark.gpu
grad = pytest.mark.grad

if torch.cuda.is_available():
    from setok_amd import _lib, ops
    from setok_amd.llama import SetokimLlamaPrefill

DEV = "cuda"
TOL = 1e-4                      # fp32 against the reference: test_llama_bwd_gpu.py's bar
LOW_VS_REFERENCE = 1.5          # 16-bit drift against fp32 may be at most this multiple of HuggingFace's own 16-bit drift (the project's convention)
DTS = [torch.float32, torch.bfloat16, torch.float16]


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _log(label, *nums):
    path = os.environ.get("SETOK_PARITY_LOG")
    if path:
        test = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]
        with open(path, "a") as f:
            f.write(f"{test}\t{label}\t" + "\t".join(f"{n:.3e}" for n in nums) + "\n")
    print(label, *[f"{n:.3e}" for n in nums])


# ======================================================================================================================================
# the kernel
# ======================================================================================================================================
def _close(got, ref, in_dt, out_dt, what):
    """The bounds tests/test_linear_abi_gpu.py::_assert_close holds setok_linear to, restated: fp32 out — max|err| / max|ref| < 2e-6 (fp32 inputs:
    the fp32 rounding class) or 2e-5 (16-bit inputs: exact products, fp32 accumulation); 16-bit out — < 6e-3 (bf16) / 1e-3 (fp16) and every element
    within one ulp of itself (2^-7 / 2^-10) plus a floor (2e-2 / 4e-3).  Returns the max-rel error."""
    got, ref = got.double(), ref.double()
    err = (got - ref).abs()
    rel = float(err.max() / ref.abs().max().clamp_min(1e-30))
    if out_dt == torch.float32:
        assert rel < (2e-6 if in_dt == torch.float32 else 2e-5), (what, rel)
        return rel
    bound, ulp, floor = (6e-3, 2.0 ** -7, 2e-2) if out_dt == torch.bfloat16 else (1e-3, 2.0 ** -10, 4e-3)
    assert rel < bound, (what, rel)
    assert bool((err <= ulp * ref.abs() + floor).all()), what
    return rel


def _operands(M, N, K, dt, seed=0):
    g = torch.Generator().manual_seed(seed * 1000003 + M * 7919 + N * 131 + K)
    a = torch.randn(M, K, generator=g).to(dt).to(DEV)
    w = (torch.randn(N, K, generator=g) * 0.5).to(dt).to(DEV)
    return a, w


@pytest.mark.parametrize("dt", DTS, ids=lambda d: str(d)[6:])
def test_linear_skinny_against_fp64(dt):
    """Every M x N x K of the grid, K on both sides of one slice and over several, alpha in {1, 2, 0.25}, both output types."""
    ks = ops.skinny_kslice(dt == torch.float16)
    worst = {}
    for K in (64, ks - 64, ks, ks + 64, 3 * ks + 128):
        for N in (16, 64, 128, 256):
            for M in (1, 31, 64, 65, 200):
                a, w = _operands(M, N, K, dt)
                ref = a.double() @ w.double().T
                for alpha in (1.0, 2.0, 0.25):
                    for od in ((dt,) if dt == torch.float32 else (dt, torch.float32)):
                        got = ops.linear_skinny(a, w, alpha=alpha, out_dtype=od)
                        assert got.dtype == od and got.shape == (M, N)
                        rel = _close(got, ref * alpha, dt, od, (M, N, K, alpha, od))
                        worst[od] = max(worst.get(od, 0.0), rel)
    for od, rel in worst.items():
        _log(f"linear_skinny {str(dt)[6:]} -> {str(od)[6:]} worst max_rel over the grid", rel)


@pytest.mark.parametrize("dt", DTS, ids=lambda d: str(d)[6:])
def test_linear_skinny_column_windows_leave_every_canary_byte(dt):
    """A and C are column windows of wider buffers (lda = K + 64, ldc = N + 24, both starting 8 / 16 columns in); W is a window too.  The result is
    the contiguous call's, bit for bit, and every byte of C's buffer outside the window — rows above and below included — is unchanged."""
    ks = ops.skinny_kslice(dt == torch.float16)
    for M, N, K in ((65, 64, ks + 64), (200, 128, 64), (31, 16, 3 * ks + 128), (129, 256, ks)):
        a, w = _operands(M, N, K, dt, seed=1)
        for od in ((dt,) if dt == torch.float32 else (dt, torch.float32)):
            want = ops.linear_skinny(a, w, alpha=2.0, out_dtype=od)
            abuf = torch.full((M, K + 64), 3.0, dtype=dt, device=DEV)
            abuf[:, 16:16 + K] = a
            wbuf = torch.full((N, K + 32), -5.0, dtype=dt, device=DEV)
            wbuf[:, 32:] = w
            cbuf = torch.full((M + 2, N + 24), 7.0, dtype=od, device=DEV)
            canary = cbuf.clone()
            win = cbuf[1:M + 1, 8:8 + N]
            assert win.stride(0) == N + 24 and abuf[:, 16:16 + K].stride(0) == K + 64
            ops.linear_skinny(abuf[:, 16:16 + K], wbuf[:, 32:], alpha=2.0, out=win, out_dtype=od)
            assert torch.equal(win, want), (M, N, K, od)
            outside = torch.ones_like(cbuf, dtype=torch.bool)
            outside[1:M + 1, 8:8 + N] = False
            assert torch.equal(cbuf.view(torch.uint8).reshape(M + 2, -1)[outside.repeat_interleave(cbuf.element_size(), dim=1)],
                               canary.view(torch.uint8).reshape(M + 2, -1)[outside.repeat_interleave(cbuf.element_size(), dim=1)]), (M, N, K, od)
            ws = torch.full((ops.linear_skinny_workspace(M, N, K, dt == torch.float16) + 64,), 9.0, dtype=torch.float32, device=DEV)
            again = ops.linear_skinny(a, w, alpha=2.0, out_dtype=od, ws=ws)               # a caller's workspace: nothing behind its stated length is written
            assert torch.equal(again, want) and bool((ws[-64:] == 9.0).all())


@pytest.mark.parametrize("dt", DTS, ids=lambda d: str(d)[6:])
def test_linear_skinny_row_bits_do_not_depend_on_the_batch_the_run_or_ldc(dt):
    ks = ops.skinny_kslice(dt == torch.float16)
    for N, K in ((128, 3 * ks + 128), (64, ks), (256, ks + 64), (16, 64)):
        a, w = _operands(200, N, K, dt, seed=2)
        full = ops.linear_skinny(a, w, alpha=0.25)
        assert torch.equal(ops.linear_skinny(a, w, alpha=0.25), full)                             # two runs
        assert torch.equal(ops.linear_skinny(a[137:138].contiguous(), w, alpha=0.25), full[137:138])      # row 137 alone, M = 1
        assert torch.equal(ops.linear_skinny(a[100:165], w, alpha=0.25), full[100:165])           # other rows around it, another row block
        wide = torch.zeros((200, N + 40), dtype=dt, device=DEV)
        ops.linear_skinny(a, w, alpha=0.25, out=wide[:, :N])                                      # a larger ldc
        assert torch.equal(wide[:, :N], full) and float(wide[:, N:].abs().max()) == 0.0
    assert ops.linear_skinny(a[:0], w).shape == (0, 16)                                           # M = 0 is a no-op


# ======================================================================================================================================
# the model against HuggingFace's autograd
# ======================================================================================================================================
def _model(name, dtype=torch.float32):
    kw, lc, seed, x, am, pos, labels, G = C.case_inputs(name)
    sd = O.init_llama_weights(lc, seed=seed)
    with torch.device("meta"):
        m = SetokimLlamaPrefill(kw)
    m = m.to_empty(device=DEV)
    assert not m.load_state_dict(sd, strict=True).missing_keys
    m = m.to(dtype).eval()
    return m, lc, seed, x, am, pos, labels


def _adapted(name, dtype, r, targets=LC.TARGETS, p=0.0):
    """The case's model with the seeded (non-zero B) adapters of lora_cases attached."""
    m, lc, seed, x, am, pos, labels = _model(name, dtype)
    m.add_lora_(r, LC.SCALING * r, target_modules=targets, lora_dropout=p)
    m.load_lora_state_dict(LC.peft_keys(LC.adapters(lc, r, seed, targets)))
    return m, lc, seed, x, am, pos, labels


def _kw(am, pos, labels):
    return dict(attention_mask=am.to(DEV), position_ids=pos.to(DEV), labels=labels.to(DEV), return_loss=True)


def _run(m, x, am, pos, labels):
    """(loss, logits, d loss / d inputs_embeds, {"{layer}.{target}.lora_A|B": gradient}) through the differentiable path."""
    m.zero_grad(set_to_none=True)
    xe = x.to(DEV).requires_grad_(True)
    logits, _, _, loss = m(inputs_embeds=xe, **_kw(am, pos, labels))
    assert loss.grad_fn is not None and logits.grad_fn is not None
    loss.backward()
    names, params = m.model.lora.flat()
    assert all(p.grad is not None and p.grad.dtype == p.dtype and p.grad.shape == p.shape for p in params)
    assert all(q.grad is None for q in list(m.model.layers.parameters()) + [m.model.norm.weight, m.lm_head.weight])
    return loss.detach(), logits.detach(), xe.grad.detach().cpu(), {n: p.grad.detach().cpu() for n, p in zip(names, params)}


@grad
@pytest.mark.parametrize("name", LC.FP32_CASES)
def test_lora_gradients_fp32_vs_hf(golden_dir, name):
    """r = 16, all seven targets: the loss, d loss / d inputs_embeds at the attended rows and every dA, dB against HuggingFace's autograd; padded
    rows exactly zero; the no_grad forward applies the adapters with the same bits and no graph."""
    z = golden_io.load(os.path.join(golden_dir, "lora.npz"))
    m, lc, seed, x, am, pos, labels = _adapted(name, torch.float32, LC.R32)
    loss, logits, dx, grads = _run(m, x, am, pos, labels)
    ref_loss = float(z[f"{name}:r16:loss"][0])
    assert abs(float(loss) - ref_loss) < TOL * abs(ref_loss)
    v = am.bool()
    parity.close(dx[v], _t(z[f"{name}:r16:dx"])[v], TOL, "d loss / d inputs_embeds")
    if (~v).any():
        assert float(dx[~v].abs().max()) == 0.0
    assert set(grads) == {k.split(":g:")[1] for k in z.files if k.startswith(f"{name}:r16:g:")}
    for n, g in grads.items():
        parity.close(g, _t(z[f"{name}:r16:g:{n}"]), TOL, n)
    with torch.no_grad():
        lg0, _, _, loss0 = m(inputs_embeds=x.to(DEV), **_kw(am, pos, labels))
        h0 = m.model(x.to(DEV), am.to(DEV), pos.to(DEV))
    assert lg0.grad_fn is None and h0.grad_fn is None and torch.equal(lg0, logits) and torch.equal(loss0, loss)
    xh = x.to(DEV).requires_grad_(True)                                     # LlamaModel.forward alone takes the same row
    h = m.model(xh, am.to(DEV), pos.to(DEV))
    assert h.grad_fn is not None and torch.equal(h, h0)
    h.float().square().sum().backward()
    assert float(xh.grad.abs().max()) > 0 and all(float(p.grad.abs().max()) > 0 for p in m.model.lora.parameters())


@grad
@pytest.mark.parametrize("dt,tag", [(torch.bfloat16, "bf16"), (torch.float16, "fp16")])
@pytest.mark.parametrize("name", LC.LOW_CASES)
def test_lora_gradients_16bit_drift_within_hfs_own(golden_dir, name, dt, tag):
    """r = 64: |GPU 16-bit gradient - HF fp32 gradient| <= 1.5 x |HF 16-bit gradient - HF fp32 gradient| in max-rel and rms-rel, for dx at the attended
    rows, all dA concatenated and all dB concatenated (HF's own 16-bit run of the same adapted model: the fixture keeps its two measures).  The
    per-tensor values are logged."""
    z = golden_io.load(os.path.join(golden_dir, "lora.npz"))
    m, lc, seed, x, am, pos, labels = _adapted(name, dt, LC.R16)
    loss, logits, dx, grads = _run(m, x, am, pos, labels)
    v = am.bool()
    ref = {n: _t(z[f"{name}:r64:g:{n}"]) for n in grads}
    for n in sorted(grads):
        gm, gr, _ = parity.measure(grads[n].float(), ref[n])
        _log(f"{name} {tag} {n}: max_rel, rms_rel", gm, gr)
    pairs = {"dx": (dx.float()[v], _t(z[f"{name}:r64:dx"])[v]),
             "dA": (LC.cat_grads(grads, "lora_A").float(), LC.cat_grads(ref, "lora_A")),
             "dB": (LC.cat_grads(grads, "lora_B").float(), LC.cat_grads(ref, "lora_B"))}
    fails = []
    for what, (got, want) in pairs.items():
        gm, gr, _ = parity.measure(got, want)
        hm, hr = (float(t) for t in z[f"{name}:r64:{tag}:{what}"])
        _log(f"{name} {tag} {what}: gpu max_rel, hf max_rel, gpu rms_rel, hf rms_rel", gm, hm, gr, hr)
        if not (gm <= LOW_VS_REFERENCE * hm and gr <= LOW_VS_REFERENCE * hr):
            fails.append((what, gm, hm, gr, hr))
    assert not fails, fails
    if (~v).any():
        assert float(dx[~v].abs().max()) == 0.0


# ======================================================================================================================================
# fresh adapters, a target subset
# ======================================================================================================================================
@grad
@pytest.mark.parametrize("dt,r", [(torch.float32, 16), (torch.bfloat16, 64)], ids=["float32", "bfloat16"])
def test_fresh_adapters_change_no_bit_and_give_zero_dA(dt, r):
    m, lc, seed, x, am, pos, labels = _model("mqa_dh128_left", dt)
    m.requires_grad_(False)
    with torch.no_grad():
        lg0, _, _, loss0 = m(inputs_embeds=x.to(DEV), **_kw(am, pos, labels))
        h0 = m.model(x.to(DEV), am.to(DEV), pos.to(DEV))
    m.add_lora_(r, 2 * r)                                                   # B = 0
    loss, logits, dx, grads = _run(m, x, am, pos, labels)
    with torch.no_grad():
        h1 = m.model(x.to(DEV), am.to(DEV), pos.to(DEV))
    assert torch.equal(h1, h0) and torch.equal(logits, lg0) and torch.equal(loss, loss0)
    assert all(float(g.abs().max()) == 0.0 for n, g in grads.items() if n.endswith("lora_A"))
    assert all(float(g.float().abs().max()) > 0.0 for n, g in grads.items() if n.endswith("lora_B"))
    assert float(dx.abs().max()) > 0


_LAYER_CALLS = ["setok_rmsnorm", "setok_linear", "setok_rope_gqa", "setok_attention_causal_gqa", "setok_linear", "setok_rmsnorm",
                "setok_linear_swiglu", "setok_linear"]                      # a prefill layer at a shape whose gate|up takes the fused launch
_FUSED = dict(hidden_size=256, intermediate_size=5888, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, vocab_size=128)


def _calls(m, x, monkeypatch):
    names, real = [], _lib.call
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "call", lambda name, *a, **k: (names.append(name), real(name, *a, **k))[1])
        with torch.no_grad():
            m.model(x)
    return names


def test_a_target_subset_keeps_the_fused_gate_up_and_no_adapters_keep_todays_calls(monkeypatch):
    """B * T = 512 rows and 2 F = 46 * 256 columns: 92 tiles, enough for linear_swiglu's single fused launch."""
    torch.manual_seed(0)
    m = SetokimLlamaPrefill(dict(_FUSED)).to(DEV).to(torch.bfloat16).eval()
    x = (torch.randn(2, 256, 256, generator=torch.Generator().manual_seed(1))).to(torch.bfloat16).to(DEV)
    plain = _calls(m, x, monkeypatch)
    assert plain == _LAYER_CALLS * 2 + ["setok_rmsnorm"]                    # exactly the calls of a prefill before adapters existed
    with torch.no_grad():
        h0 = m.model(x)
    m.add_lora_(64, 128, target_modules=("q_proj", "v_proj"))
    pair = ["setok_linear_skinny", "setok_linear"]
    want = ["setok_rmsnorm", "setok_linear"] + pair + pair + _LAYER_CALLS[2:]
    assert _calls(m, x, monkeypatch) == want * 2 + ["setok_rmsnorm"]
    with torch.no_grad():
        assert torch.equal(m.model(x), h0)                                  # (fresh: B = 0)
    m2 = SetokimLlamaPrefill(dict(_FUSED)).to(DEV).to(torch.bfloat16).eval()
    m2.add_lora_(64, 128, target_modules=("up_proj",))
    names = _calls(m2, x, monkeypatch)
    assert "setok_linear_swiglu" not in names and names.count("setok_swiglu_pairs") == 2 and names.count("setok_linear_skinny") == 2


# ======================================================================================================================================
# dropout
# ======================================================================================================================================
@grad
def test_dropout_masks_are_a_function_of_seed_and_offset_and_eval_ignores_p():
    """p = 0.25 in training mode, tiny_left, fp32: the masks read back from ops.dropout on ones with the run's (seed, offset) and put into a float64
    torch restatement (HF's Llama in float64 with the LoRA rule around its Linears) give the reference gradients."""
    name, p = "tiny_left", 0.25
    m, lc, seed, x, am, pos, labels = _adapted(name, torch.float32, LC.R32, p=p)
    m.train()
    torch.manual_seed(1234)
    loss, logits, dx, grads = _run(m, x, am, pos, labels)
    ad = m.model.lora
    assert ad.seed is not None
    rows = x.shape[0] * x.shape[1]
    masks = {}
    for i in range(lc.num_hidden_layers):
        for t in LC.TARGETS:
            fan_in = LC.shapes(lc)[t][1]
            kept = ops.dropout(torch.ones(rows, fan_in, device=DEV), p, ad.seed, ad.dropout_offset(i, t))
            assert bool(((kept == 0) | ((kept - 1 / (1 - p)).abs() < 1e-6)).all())
            masks[f"{i}.{t}"] = (kept != 0).cpu()
            assert 0.6 < float(masks[f"{i}.{t}"].float().mean()) < 0.9
    assert not torch.equal(masks["0.q_proj"], masks["0.k_proj"]) and not torch.equal(masks["0.q_proj"], masks["1.q_proj"])       # its own offset each
    kw_, _, _, _, _, _, _, _ = C.case_inputs(name)
    hf = LC.hf_llama(kw_, lc, O.init_llama_weights(lc, seed=seed), torch.float64)
    wrapped = LC.wrap_hf(hf, LC.adapters(lc, LC.R32, seed), LC.SCALING, torch.float64, masks=masks, p=p)
    with torch.enable_grad():
        xe = x.double().requires_grad_(True)
        ref_loss = LC.lm_loss(hf(inputs_embeds=xe, attention_mask=LC.additive_mask(am, torch.float64), position_ids=pos).logits, labels, am)
        ref_loss.backward()
    assert abs(float(loss) - float(ref_loss)) < TOL * abs(float(ref_loss))
    v = am.bool()
    parity.close(dx[v], xe.grad[v], TOL, "dropout: d loss / d inputs_embeds")
    for k, mod in wrapped.items():
        parity.close(grads[k + ".lora_A"], mod.lora_A.grad, TOL, "dropout: " + k + ".lora_A")
        parity.close(grads[k + ".lora_B"], mod.lora_B.grad, TOL, "dropout: " + k + ".lora_B")
    loss2, _, dx2, _ = _run(m, x, am, pos, labels)                          # another seed, other masks
    assert float(loss2) != float(loss)
    # eval(): the identity, bit for bit
    m.eval()
    loss_e, logits_e, dx_e, grads_e = _run(m, x, am, pos, labels)
    assert ad.seed is None
    m0, _, _, _, _, _, _ = _adapted(name, torch.float32, LC.R32, p=0.0)
    loss_0, logits_0, dx_0, grads_0 = _run(m0, x, am, pos, labels)
    assert torch.equal(loss_e, loss_0) and torch.equal(logits_e, logits_0) and torch.equal(dx_e, dx_0)
    assert all(torch.equal(grads_e[n], grads_0[n]) for n in grads_0)


# ======================================================================================================================================
# a short training run, merging, refusals
# ======================================================================================================================================
@grad
def test_ten_adamw_steps_on_the_adapters_lower_the_loss(golden_dir):
    z = golden_io.load(os.path.join(golden_dir, "lora.npz"))
    m, lc, seed, x, am, pos, labels = _adapted("tiny_left", torch.float32, LC.R32)
    opt = torch.optim.AdamW(m.model.lora.parameters(), lr=1e-2)
    losses = []
    for _ in range(11):
        opt.zero_grad(set_to_none=True)
        _, _, _, loss = m(inputs_embeds=x.to(DEV), **_kw(am, pos, labels))   # inputs_embeds without a gradient: the adapters alone train
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    ref = float(z["tiny_left:r16:loss"][0])
    assert abs(losses[0] - ref) < TOL * abs(ref)
    assert losses[10] < losses[0], losses
    _log("ten AdamW steps: loss at step 0, step 10", losses[0], losses[10])


def test_merge_lora_fp32_bf16_and_generate_after_it():
    name = "mqa_dh128_left"
    m, lc, seed, x, am, pos, labels = _adapted(name, torch.float32, 64)
    kw = dict(attention_mask=am.to(DEV), position_ids=pos.to(DEV))
    with torch.no_grad():
        before = m(inputs_embeds=x.to(DEV), **kw)[0]
    w_q = m.model.layers[0].self_attn.q_proj.weight.detach().clone()
    assert m.merge_lora_() is m and m.model.lora is None
    assert not any("lora" in k for k in m.state_dict()) and not torch.equal(m.model.layers[0].self_attn.q_proj.weight, w_q)
    with torch.no_grad():
        merged32 = m(inputs_embeds=x.to(DEV), **kw)[0]
    v = am.bool()
    parity.close(merged32[v.to(DEV)], before[v.to(DEV)], 1e-4, "fp32 logits: merged against the adapter forward")
    out = m.generate(inputs_embeds=x.to(DEV), attention_mask=am.to(DEV), max_new_tokens=3)
    assert out.shape == (x.shape[0], 3)
    with pytest.raises(ValueError, match="no adapters are attached"):
        m.merge_lora_()
    # bf16: the merged weights are rounded once; the unmerged bf16 forward is the yardstick
    mb, _, _, _, _, _, _ = _adapted(name, torch.bfloat16, 64)
    with torch.no_grad():
        unmerged = mb(inputs_embeds=x.to(DEV), **kw)[0]
    mb.merge_lora_()
    with torch.no_grad():
        merged16 = mb(inputs_embeds=x.to(DEV), **kw)[0]
    ref = merged32.cpu()[v]
    gm, gr, _ = parity.measure(merged16.float().cpu()[v], ref)
    ym, yr, _ = parity.measure(unmerged.float().cpu()[v], ref)
    _log("bf16 logits vs fp32 merged: merged max_rel, unmerged max_rel, merged rms_rel, unmerged rms_rel", gm, ym, gr, yr)
    assert gm <= LOW_VS_REFERENCE * ym and gr <= LOW_VS_REFERENCE * yr, (gm, ym, gr, yr)
    assert mb.generate(inputs_embeds=x.to(DEV), attention_mask=am.to(DEV), max_new_tokens=2).shape == (x.shape[0], 2)
    assert not any("lora" in k for k in mb.state_dict())


@grad
def test_refusals_with_unmerged_adapters_and_on_the_training_path():
    from setok_amd.generation import KVCache
    m, lc, seed, x, am, pos, labels = _adapted("tiny_left", torch.float32, LC.R32)
    xd = x.to(DEV)
    B, T, D = xd.shape
    cache = KVCache.for_model(m.model, B, T + 4, DEV)
    for what, call in (("generate", lambda: m.generate(inputs_embeds=xd, max_new_tokens=2)),
                       ("prefill", lambda: m.model.prefill(xd, am.to(DEV), pos.to(DEV), cache)),
                       ("decode_step", lambda: m.model.decode_step(xd[:, 0], cache)),
                       ("extend", lambda: m.model.extend(xd, cache)),
                       ("quantize_fp8_", lambda: m.quantize_fp8_())):
        with pytest.raises(NotImplementedError, match=what + r".*merge_lora_\(\)"):
            call()
    assert cache.len == 0 and m.weight_format == "native"
    # last_token_only stays inference-only on the training path, with adapters and without
    for mm in (m, _model("tiny_left")[0].requires_grad_(False)):
        xe = xd.clone().requires_grad_(True)
        last, _, _ = mm(inputs_embeds=xe, attention_mask=am.to(DEV), position_ids=pos.to(DEV), last_token_only=True)
        with pytest.raises(NotImplementedError, match="last_token_only.*inference-only"):
            last.sum().backward()
    # a stack parameter that requires a gradient next to adapters: the forward runs (adapters applied), backward raises the existing message
    with torch.no_grad():
        ref = m(inputs_embeds=xd, **_kw(am, pos, labels))[3]
    m.model.layers[1].mlp.down_proj.weight.requires_grad_(True)
    xe = xd.clone().requires_grad_(True)
    loss = m(inputs_embeds=xe, **_kw(am, pos, labels))[3]
    assert torch.equal(loss.detach(), ref)
    with pytest.raises(NotImplementedError, match="SetokimLlamaPrefill.*freeze the LLM to train through it"):
        loss.backward()
    h = m.model(xe, am.to(DEV), pos.to(DEV))
    with pytest.raises(NotImplementedError, match="LlamaModel.*freeze the LLM to train through it"):
        h.sum().backward()
    assert xe.grad is None and all(p.grad is None for p in m.model.lora.parameters())
