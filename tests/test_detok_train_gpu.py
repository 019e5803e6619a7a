"""Backward pass of the reconstruction decoder (SetokDeTokenizer: forward, decode_image, reconstruction_loss; detok_train.py) on a real MI355X,
against torch autograd through the CPU oracle (oracle.detokenizer_forward + unpatchify + pixel_loss are plain torch), and the attention
backward kernel (ops.mha_bwd) against torch autograd of fp32 attention.  `pytest -m gpu`."""
import math
import os

import numpy as np
import pytest
import torch

import golden_io
import setok_oracle as O
from parity import close, measure

pytestmark = [pytest.mark.gpu, pytest.mark.grad]

if torch.cuda.is_available():
    from setok_amd import SetokDeTokenizer, ops
    from setok_amd.tokenizer import RaggedTokens

DEV = "cuda"


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _case(golden_dir, name):
    z = golden_io.load(os.path.join(golden_dir, "detok.npz"))
    kw = {str(k): v for k, v in zip(z[name + ":cfg_keys"], z[name + ":cfg_vals"])}
    kw = {k: (float(v) if k == "mlp_ratio" else int(v)) for k, v in kw.items()}
    dc = O.DetokConfig(**kw)
    sd = O.init_detok_weights(dc, seed=int(z[name + ":seed"]))
    g = torch.Generator().manual_seed(11)
    n_out = dc.patch_size ** 2 * 3
    sd["to_pixels.weight"] = (torch.rand(n_out, dc.decoder_embed_dim, generator=g) * 2 - 1) * math.sqrt(6.0 / (n_out + dc.decoder_embed_dim))
    sd["to_pixels.bias"] = torch.randn(n_out, generator=g) * 0.02
    B = z[name + ":x"].shape[0]
    gold = torch.randn(B, 3, dc.image_size, dc.image_size, generator=g) * 0.5
    return dc, sd, _t(z[name + ":x"]).float(), _t(z[name + ":mask"]).float(), gold


def _build(dc, sd, dtype=torch.float32, **kw):
    det = SetokDeTokenizer(token_feat_dim=dc.token_feat_dim, hidden_dim=dc.hidden_dim, patch_size=dc.patch_size,
                           image_size=dc.image_size, decoder_embed_dim=dc.decoder_embed_dim, decoder_nheads=dc.decoder_nheads,
                           decoder_depth=dc.decoder_depth, mlp_ratio=dc.mlp_ratio,
                           feature_mapper_path_or_name=dict(hidden_size=dc.mapper_hidden, num_attention_heads=dc.mapper_heads,
                                                            intermediate_size=dc.mapper_intermediate, layer_norm_eps=dc.mapper_eps),
                           num_hidden_layers=dc.num_hidden_layers, cross_attention_freq=dc.cross_attention_freq, pixel_head=True, **kw)
    res = det.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and set(res.missing_keys) <= {"position_embedding.inv_freq"}
    return det.to(device=DEV, dtype=dtype).eval()


def _oracle_grads(dc, sd, x, mask, gold, kind, dtype):
    """torch autograd of the oracle's decoder + pixel head + loss on CPU in `dtype`: (loss, {name: grad}, d x)."""
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    xx = x.to(dtype).clone().requires_grad_(True)
    out = O.detokenizer_forward(p, dc, xx, mask.to(dtype))
    B, Q, D = out.shape
    patches = torch.nn.functional.linear(out.reshape(B * Q, D), p["to_pixels.weight"], p["to_pixels.bias"])
    img = O.unpatchify(patches, B, dc.grid, dc.grid, dc.patch_size)
    loss = O.pixel_loss(img, gold.to(dtype), kind)
    loss.backward()
    return loss.detach(), {k: v.grad for k, v in p.items()}, xx.grad


def _run(det, x, mask, gold, kind):
    det.zero_grad(set_to_none=True)
    xx = x.to(device=DEV, dtype=det.dtype).clone().requires_grad_(True)
    loss = det.reconstruction_loss(xx, gold.to(DEV), mask.to(DEV), kind=kind)
    loss.backward()
    return loss.detach(), {n: p.grad for n, p in det.named_parameters()}, xx.grad


# ---- 1. fp32 gradient parity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mse", "l1"])
@pytest.mark.parametrize("name", ["small", "bertbase"])
def test_fp32_gradients_match_oracle_autograd(golden_dir, name, kind):
    dc, sd, x, mask, gold = _case(golden_dir, name)
    det = _build(dc, sd)
    loss, got, dx = _run(det, x, mask, gold, kind)
    ref_loss, ref, ref_dx = _oracle_grads(dc, sd, x, mask, gold, kind, torch.float64)
    close(loss.reshape(1), ref_loss.reshape(1), 1e-4, "loss")
    assert set(got) == set(ref), set(got) ^ set(ref)
    for n in ref:
        assert got[n] is not None and got[n].shape == ref[n].shape and got[n].dtype == torch.float32, n
        if n.endswith("self.key.bias"):                                       # exactly zero (a softmax row is shift-invariant): rounding noise only
            assert float(got[n].abs().max()) < 1e-4 * float(ref[n[:-4] + "weight"].abs().max()), n
            continue
        close(got[n], ref[n], 1e-4, n)
    m = mask.to(DEV).bool()
    close(dx[m], ref_dx[mask.bool()], 1e-4, "d tokens")
    assert torch.equal(dx[~m], torch.zeros_like(dx[~m]))                     # masked positions: exact zeros


# ---- 2. 16-bit gradient parity (head dims 48 and 64) ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_16bit_gradients_within_the_oracles_own_16bit_error(golden_dir, dtype):
    dc, sd, x, mask, gold = _case(golden_dir, "bertbase")
    det = _build(dc, sd, dtype)
    _, got, dx = _run(det, x, mask, gold, "mse")
    _, ref, ref_dx = _oracle_grads(dc, sd, x, mask, gold, "mse", torch.float64)
    _, low, low_dx = _oracle_grads(dc, sd, x, mask, gold, "mse", dtype)
    got["d tokens"], ref["d tokens"], low["d tokens"] = dx[mask.to(DEV).bool()], ref_dx[mask.bool()], low_dx[mask.bool()]
    bad = {}
    for n in ref:
        if n.endswith("self.key.bias"):                                       # exactly zero in exact arithmetic: no relative error to compare
            continue
        ours, theirs = measure(got[n].float(), ref[n]), measure(low[n].float(), ref[n])      # (max, rms, element-wise) against fp64
        for what, a, b in zip(("max", "rms", "elem"), ours, theirs):
            print(f"{dtype} {n} {what}: ours {a:.3e} oracle-{dtype} {b:.3e} ratio {a / max(b, 1e-30):.2f}")
            if a > 1.5 * b:
                bad[f"{n} {what}"] = (a, b)
    assert not bad, bad


# ---- 3. the attention backward kernel ------------------------------------------------------------------------------------------------
def _attn_ref(q, k, v, dout, q_len, offs, scale):
    """torch autograd of fp32 attention per segment: (dq, dk, dv) on the same (16-bit) inputs."""
    q, k, v = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    H, Dh = _attn_ref.H, _attn_ref.Dh
    outs = []
    for s in range(len(offs) - 1):
        qs = q[s * q_len:(s + 1) * q_len].reshape(q_len, H, Dh).transpose(0, 1)
        ks = k[offs[s]:offs[s + 1]].reshape(-1, H, Dh).transpose(0, 1)
        vs = v[offs[s]:offs[s + 1]].reshape(-1, H, Dh).transpose(0, 1)
        outs.append((torch.softmax(qs @ ks.transpose(1, 2) * scale, -1) @ vs).transpose(0, 1).reshape(q_len, H * Dh))
    torch.cat(outs).backward(dout.float())
    return q.grad, k.grad, v.grad


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("Dh", [48, 64])
@pytest.mark.parametrize("q_len", [25, 256, 324])
def test_mha_bwd_self_attention_on_qkv_windows(monkeypatch, dtype, Dh, q_len):
    H, B = 2, 2
    C = H * Dh
    g = torch.Generator().manual_seed(q_len + Dh)
    qkv = torch.randn(B * q_len, 3 * C, generator=g).to(device=DEV, dtype=dtype)
    scale = Dh ** -0.5
    out = ops.attention(qkv, H, Dh, scale, seg_len=q_len)
    dout = torch.randn(B * q_len, C, generator=g).to(device=DEV, dtype=dtype)
    dqkv = torch.empty_like(qkv)
    ops.mha_bwd(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], out, dout, H, Dh, scale, q_len, None, B, q_len,
                dq=dqkv[:, :C], dk=dqkv[:, C:2 * C], dv=dqkv[:, 2 * C:])
    _attn_ref.H, _attn_ref.Dh = H, Dh
    ref = _attn_ref(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], dout, q_len, [s * q_len for s in range(B + 1)], scale)
    tol = {torch.bfloat16: 3e-2, torch.float16: 1e-2, torch.float32: 1e-4}[dtype]
    for i, r in enumerate(ref):
        close(dqkv[:, i * C:(i + 1) * C].float(), r, tol, ("dq", "dk", "dv")[i])
    # the generic form (SETOK_ATTN_BWD_GENERIC=1; fp32 has no other): close to the MFMA kernel, and the same bits as setok_attention_bwd, whose
    # generic branch runs the same kernels with the self-attention row lookup
    monkeypatch.setenv("SETOK_ATTN_BWD_GENERIC", "1")
    gen = torch.empty_like(qkv)
    ops.mha_bwd(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], out, dout, H, Dh, scale, q_len, None, B, q_len,
                dq=gen[:, :C], dk=gen[:, C:2 * C], dv=gen[:, 2 * C:])
    assert torch.equal(gen, ops.attention_bwd(qkv, out, dout, H, Dh, scale, q_len))
    monkeypatch.delenv("SETOK_ATTN_BWD_GENERIC")
    for i in range(3):
        close(dqkv[:, i * C:(i + 1) * C].float(), gen[:, i * C:(i + 1) * C].float(), tol, ("dq", "dk", "dv")[i] + " vs generic")
    # two runs: the same bits
    again = torch.empty_like(qkv)
    ops.mha_bwd(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], out, dout, H, Dh, scale, q_len, None, B, q_len,
                dq=again[:, :C], dk=again[:, C:2 * C], dv=again[:, 2 * C:])
    assert torch.equal(dqkv, again)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("Dh", [48, 64])
def test_mha_bwd_cross_attention_ragged(monkeypatch, dtype, Dh):
    H, q_len = 2, 25
    C = H * Dh
    lens = [1, 31, 32, 33, 256]
    B = len(lens)
    offs = [0]
    for n in lens:
        offs.append(offs[-1] + n)
    g = torch.Generator().manual_seed(Dh)
    q = torch.randn(B * q_len, C, generator=g).to(device=DEV, dtype=dtype)
    kv = torch.randn(offs[-1], 2 * C, generator=g).to(device=DEV, dtype=dtype)
    kv_off = torch.tensor(offs, dtype=torch.int32, device=DEV)
    scale = 1.0 / math.sqrt(Dh)
    out = ops.cross_attention(q, kv[:, :C], kv[:, C:], H, Dh, scale, q_len, kv_off, B, max(lens))
    dout = torch.randn(B * q_len, C, generator=g).to(device=DEV, dtype=dtype)
    dq, dk, dv = ops.mha_bwd(q, kv[:, :C], kv[:, C:], out, dout, H, Dh, scale, q_len, kv_off, B, max(lens))
    _attn_ref.H, _attn_ref.Dh = H, Dh
    ref = _attn_ref(q, kv[:, :C], kv[:, C:], dout, q_len, offs, scale)
    tol = {torch.bfloat16: 3e-2, torch.float16: 1e-2, torch.float32: 1e-4}[dtype]
    for got, r, n in zip((dq, dk, dv), ref, ("dq", "dk", "dv")):
        close(got.float(), r, tol, n)
    dq2, dk2, dv2 = ops.mha_bwd(q, kv[:, :C], kv[:, C:], out, dout, H, Dh, scale, q_len, kv_off, B, max(lens))
    assert torch.equal(dq, dq2) and torch.equal(dk, dk2) and torch.equal(dv, dv2)
    monkeypatch.setenv("SETOK_ATTN_BWD_GENERIC", "1")                        # against the generic kernels
    gen = ops.mha_bwd(q, kv[:, :C], kv[:, C:], out, dout, H, Dh, scale, q_len, kv_off, B, max(lens))
    monkeypatch.delenv("SETOK_ATTN_BWD_GENERIC")
    for got, r, n in zip((dq, dk, dv), gen, ("dq", "dk", "dv")):
        close(got.float(), r.float(), tol, n + " vs generic")
    with pytest.raises(AssertionError, match="max_kv"):                       # a segment longer than max_kv is refused, not half written
        ops.mha_bwd(q, kv[:, :C], kv[:, C:], out, dout, H, Dh, scale, q_len, kv_off, B, 255)
    # one segment alone == the same segment inside the batch
    s = 3
    one = torch.tensor([0, lens[s]], dtype=torch.int32, device=DEV)
    qs, kvs, os_, ds = (q[s * q_len:(s + 1) * q_len].contiguous(), kv[offs[s]:offs[s + 1]].contiguous(),
                        out[s * q_len:(s + 1) * q_len].contiguous(), dout[s * q_len:(s + 1) * q_len].contiguous())
    a, b, c = ops.mha_bwd(qs, kvs[:, :C], kvs[:, C:], os_, ds, H, Dh, scale, q_len, one, 1, lens[s])
    assert torch.equal(a, dq[s * q_len:(s + 1) * q_len]) and torch.equal(b, dk[offs[s]:offs[s + 1]]) and torch.equal(c, dv[offs[s]:offs[s + 1]])


def test_pixel_loss_bwd_matches_autograd():
    g = torch.Generator().manual_seed(5)
    B, gh, p, n_pad = 2, 3, 14, 640
    patches = torch.randn(B * gh * gh, n_pad, generator=g).to(DEV)
    gold = torch.randn(B, 3, gh * p, gh * p, generator=g).to(DEV)
    gold[0, 0, 0, 0] = 0.0
    patches[0, 0] = 0.0                                                      # pred == gold at one pixel: sign(0) = 0
    for kind in ("mse", "l1"):
        pt = patches.clone().requires_grad_(True)
        O.pixel_loss(O.unpatchify(pt[:, :3 * p * p], B, gh, gh, p), gold, kind).backward()
        img = ops.unpatchify(patches, B, gh, gh, p)
        up = torch.tensor(1.0, device=DEV)
        got = ops.pixel_loss_bwd(img, gold, kind, up, n_pad, gh, gh, p)
        close(got, pt.grad, 1e-6, kind)
        assert torch.equal(got[:, 3 * p * p:], torch.zeros_like(got[:, 3 * p * p:]))
    img = ops.unpatchify(patches, B, gh, gh, p)
    img[1, 2, 3, 4] = float("nan")                                           # torch.sign(NaN) = NaN: the gradient propagates it
    got = ops.pixel_loss_bwd(img, gold, "l1", torch.tensor(1.0, device=DEV), n_pad, gh, gh, p)
    assert int(torch.isnan(got).sum()) == 1


# ---- 4. behaviour kept ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,fold", [(torch.float32, "1"), (torch.bfloat16, "1"), (torch.bfloat16, "0")])
def test_grad_recording_forward_returns_the_no_grad_values(golden_dir, monkeypatch, dtype, fold):
    monkeypatch.setenv("SETOK_LN_FOLD", fold)
    dc, sd, x, mask, gold = _case(golden_dir, "bertbase")
    det = _build(dc, sd, dtype)
    xx, mm, gg = x.to(device=DEV, dtype=dtype), mask.to(DEV), gold.to(DEV)
    with torch.no_grad():
        f0, i0, l0 = det(xx, mm), det.decode_image(xx, mm), det.reconstruction_loss(xx, gg, mm)
    f1, i1, l1 = det(xx, mm), det.decode_image(xx, mm), det.reconstruction_loss(xx, gg, mm)
    assert f1.grad_fn is not None and i1.grad_fn is not None and l1.grad_fn is not None
    assert torch.equal(f0, f1) and torch.equal(i0, i1) and torch.equal(l0, l1)
    (f1.float().square().mean() + i1.float().mean() + l1).backward()         # all three entry points differentiate
    assert all(p.grad is not None and bool(torch.isfinite(p.grad.float()).all()) for p in det.parameters())


def test_training_mode_dropout_still_refuses_the_backward_pass(golden_dir):
    dc, sd, x, mask, gold = _case(golden_dir, "small")
    det = _build(dc, sd).train()                                            # default proj_drop = attn_drop = 0.2
    loss = det.reconstruction_loss(x.to(DEV), gold.to(DEV), mask.to(DEV))
    with pytest.raises(NotImplementedError, match="training-mode dropout in the decoder"):
        loss.backward()
    det0 = _build(dc, sd, proj_drop=0.0, attn_drop=0.0).train()            # zero rates: real gradients in training mode
    det0.reconstruction_loss(x.to(DEV), gold.to(DEV), mask.to(DEV)).backward()
    assert det0.mapper_fc_in.weight.grad is not None
    with pytest.raises(ValueError, match="gold_image requires a gradient"):
        det0.reconstruction_loss(x.to(DEV), gold.to(DEV).requires_grad_(True), mask.to(DEV))


def test_frozen_decoder_gives_token_gradients_only(golden_dir):
    dc, sd, x, mask, gold = _case(golden_dir, "small")
    det = _build(dc, sd).requires_grad_(False)
    counts = mask.sum(1).long().tolist()
    rows = torch.cat([x[i, :c] for i, c in enumerate(counts)]).to(DEV).requires_grad_(True)
    det.reconstruction_loss(RaggedTokens(rows, counts), gold.to(DEV)).backward()
    assert rows.grad is not None and float(rows.grad.abs().max()) > 0
    assert all(p.grad is None for p in det.parameters())
    det2 = _build(dc, sd)                                                   # the same d(tokens) as with a trainable decoder
    r2 = rows.detach().clone().requires_grad_(True)
    det2.reconstruction_loss(RaggedTokens(r2, counts), gold.to(DEV)).backward()
    assert torch.equal(rows.grad, r2.grad)


# ---- 5. stage 1: tokenizer head -> decoder -> pixel loss in one graph -------------------------------------------------------------
def test_stage1_chain_from_the_tokenizer_head(golden_dir):
    from setok_amd import SetokTokenizer
    from setok_amd.training import head_backward, head_forward_train
    z = golden_io.load(os.path.join(golden_dir, "head_small.npz"))
    gz = golden_io.load(os.path.join(golden_dir, "head_grads.npz"))
    hsd = {k[2:]: _t(z[k]) for k in z.files if k.startswith("w:")}
    hidden = torch.cat([torch.cat([torch.zeros(1, 64), _t(z[f"{n}:feats"])], 0) for n in ("dynamic", "planted")], 0).to(DEV)
    thr = float(gz["threshold"])
    tok = SetokTokenizer(vision_tower=dict(hidden_size=64, intermediate_size=128, num_hidden_layers=3, num_attention_heads=4, image_size=112,
                                           patch_size=14), mm_vision_select_layer=-2, hidden_dim=64, token_feat_dim=96, min_cluster_num=8,
                         threshold=0.5, nheads=2, dim_feedforward=128)
    assert not tok.load_state_dict(hsd, strict=False).unexpected_keys
    tok = tok.to(DEV).eval()
    dc, sd, _, _, _ = _case(golden_dir, "small")
    det = _build(dc, sd)
    gold = torch.randn(2, 3, dc.image_size, dc.image_size, generator=torch.Generator().manual_seed(8)).to(DEV)

    feats, _, _ = tok.encode_features(hidden, 2, threshold=thr)
    det.reconstruction_loss(feats, gold).backward()
    head = {n: p.grad.clone() for n, p in tok.named_parameters() if p.grad is not None}
    dec = {n: p.grad.clone() for n, p in det.named_parameters()}
    assert head and all(v is not None for v in dec.values())

    det.zero_grad(set_to_none=True)
    packed = feats.packed.detach().clone().requires_grad_(True)             # the decoder alone on the same tokens
    det.reconstruction_loss(RaggedTokens(packed, feats.counts), gold).backward()
    for n, p in det.named_parameters():
        assert torch.equal(p.grad, dec[n]), n
    with torch.no_grad():
        tokens, ctx = head_forward_train(tok, hidden, 2, threshold=thr)
        want = head_backward(tok, ctx, packed.grad)
    assert torch.equal(tokens.packed, feats.packed)
    for n, gr in head.items():
        assert torch.equal(gr, want[n].to(gr.dtype).reshape(gr.shape)), n
