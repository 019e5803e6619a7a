"""Pin of the oracle against the reference's own code (RAC).  The reference's side is recorded in tests/golden/reference_live.npz
(`python tests/golden/make_golden.py reference_live`: the reference's modules run on the inputs these tests build, which are seeded and
regenerated here bit-exactly, plus the small tokenizer's weights and state-dict layout); the oracle's side runs live.  The `_live` in
some test names is the oracle's side: what they compare it with is the reference's recorded output."""
import hashlib
import os

import numpy as np
import pytest
import torch

import golden_io
import setok_oracle as O

torch.set_num_threads(min(8, os.cpu_count() or 1))


@pytest.fixture(scope="module")
def tok(golden_dir):
    """The reference's side: the small reference tokenizer (hidden 64, 3 layers, token_feat_dim 96) and its recorded outputs."""
    return golden_io.load(os.path.join(golden_dir, "reference_live.npz"))


def _t(z, key):
    return torch.from_numpy(np.array(z[key]))


def _sd(tok):
    return {k[2:]: _t(tok, k) for k in tok.files if k.startswith("w:")}


HC = O.HeadConfig(hidden_dim=64, token_feat_dim=96, min_cluster_num=8, threshold=0.5, nheads=2, dim_feedforward=128)
VC = O.VitConfig(64, 128, 3, 4, 112, 14)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_head_bitwise_on_identical_features(tok, seed):
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(64, 64, generator=g)
    noise = torch.rand(64, generator=g)
    thr = float(tok[f"head:{seed}:thr"])                       # from the reference's own scores (ranks 11-12)
    for j, kw in enumerate((dict(), dict(threshold=thr), dict(k=5, threshold=thr))):
        ref = {name: _t(tok, f"head:{seed}:{j}:{name}") for name in ("x", "index_down", "idx_cluster", "score", "tokens")}
        got = O.head_forward(_sd(tok), HC, feats, noise=noise, **kw)
        assert torch.equal(ref["x"], got.x)
        assert torch.equal(ref["index_down"], got.index_down)
        assert torch.equal(ref["idx_cluster"], got.idx_cluster)
        assert torch.equal(ref["score"], got.score)            # same formula, same torch kernels
        assert torch.equal(ref["tokens"], got.tokens)


def test_cdist_restatement_is_bitwise(tok):
    g = torch.Generator().manual_seed(9)
    for n, c in ((26, 8), (256, 1024), (576, 256)):
        x = torch.randn(n, c, generator=g)
        assert torch.equal(torch.cdist(x, x), O.pairwise_dist(x))


def test_tower_restatement_vs_hf(tok):
    g = torch.Generator().manual_seed(3)
    images = torch.randn(2, 3, 112, 112, generator=g)
    for sel in (-2, -1, 1):
        ref = _t(tok, f"tower:{sel}")                          # the reference's CLIPVisionTower (HF CLIP) at this layer selection
        got = O.tower_forward(_sd(tok), VC, images, sel)
        torch.testing.assert_close(got, ref, rtol=1e-5, atol=5e-6)


def test_pos_encoding_bitwise(tok):
    """The reference's PositionalEncoding2D tables: the small one stored whole, every one as the SHA-256 of its float32 bytes."""
    for h, w, c in ((16, 16, 1024), (24, 24, 1024), (14, 14, 768), (3, 5, 10)):
        got = O.pos_encoding_2d(h, w, c)
        assert got.dtype == torch.float32 and tuple(got.shape) == (h * w, c)
        if f"pe:{h}x{w}x{c}" in tok:
            assert torch.equal(_t(tok, f"pe:{h}x{w}x{c}"), got)
        digest = np.frombuffer(hashlib.sha256(got.contiguous().numpy().tobytes()).digest(), np.uint8)
        assert np.array_equal(digest, tok[f"pe_sha256:{h}x{w}x{c}"]), (h, w, c)


def test_reference_defects_recorded(tok):
    """D1/D2 of SURVEY.md §0.2 — documents why RAC needs its two repairs: the recorded run of the reference's forward raised on a batch of
    two images (D1) and its inter_encoder on a 2-D input (ValueError, D2); the oracle, which loops over the images, encodes the same batch."""
    assert str(tok["defect:D1"]) != ""
    assert str(tok["defect:D2"]) == "ValueError"
    feats, res = O.encode(_sd(tok), VC, HC, torch.randn(2, 3, 112, 112, generator=torch.Generator().manual_seed(0)))
    assert feats.shape[0] == 2 and len(res) == 2 and all(r.tokens.shape[1] == 96 for r in res)


def test_qformer_restatement_vs_reference_live(tok):
    """a9: oracle.qformer_forward against the recorded output of the reference's BertEmbeddings + BertEncoder (module.py:151-690)."""
    dc = O.DetokConfig(token_feat_dim=48, hidden_dim=32, patch_size=14, image_size=42, decoder_embed_dim=32, decoder_nheads=2,
                       decoder_depth=1, num_hidden_layers=3, cross_attention_freq=2, mapper_hidden=32, mapper_heads=4,
                       mapper_intermediate=64)
    sd = O.init_detok_weights(dc, seed=11)
    torch.manual_seed(0)
    x = torch.randn(3, 6, 32)
    mask = torch.ones(3, 6); mask[0, 2:] = 0; mask[2, 5:] = 0
    q = sd["mask_tokens"].expand(3, -1, -1)
    ref = _t(tok, "qformer:mask")
    got = O.qformer_forward(sd, dc, q, x, mask)
    torch.testing.assert_close(got, ref, rtol=1e-6, atol=1e-6)
    ref_nomask = _t(tok, "qformer:nomask")
    torch.testing.assert_close(O.qformer_forward(sd, dc, q, x, None), ref_nomask, rtol=1e-6, atol=1e-6)


KWS = [dict(), dict(padding_side="left"), dict(max_length=11), dict(max_length=5, padding_side="left")]


@pytest.mark.parametrize("kw", KWS)
def test_splice_restatement_vs_reference_live(tok, kw):
    """§8(f) row 1: oracle.splice_multimodal against the recorded outputs of the reference's prepare_inputs_labels_for_multimodal
    (setokim_arch.py:213-355) executed unmodified; every output tensor bit-equal, None conventions included."""
    ids, am, labels, feats, W = O.splice_inputs(21, 6, 14, 50, 12)
    pos = torch.arange(14).expand(6, 14).clone()
    i = KWS.index(kw)
    for v, (p_, a_, l_) in enumerate(((pos, am, labels), (None, None, None), (None, am.bool(), labels), (pos, am, None))):
        n = int(tok[f"splice:{i}:{v}:n"])
        ref = [_t(tok, f"splice:{i}:{v}:{j}") if f"splice:{i}:{v}:{j}" in tok else None for j in range(n)]
        got = O.splice_multimodal(ids, p_, a_, l_, feats, W, **kw)
        assert len(got) == n
        for r, g in zip(ref, got):
            assert (r is None) == (g is None)
            if r is not None:
                assert r.dtype == g.dtype and torch.equal(r, g)


def test_llama_restatement_vs_installed_hf_live():
    """cfg 5: oracle.llama_forward against the installed HuggingFace LlamaForCausalLM (third-party arithmetic the reference calls at
    setokim_llama.py:130-143), eager attention, fp32 — bit-equal on token positions."""
    from transformers import LlamaConfig, LlamaForCausalLM
    kw = dict(hidden_size=64, intermediate_size=176, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4, vocab_size=100)
    lc = O.LlamaConfigLite(**kw)
    sd = O.init_llama_weights(lc, seed=3)
    cfg = LlamaConfig(**kw, rms_norm_eps=lc.rms_norm_eps, rope_theta=lc.rope_theta, attention_bias=False, mlp_bias=False, tie_word_embeddings=False)
    cfg._attn_implementation = "eager"
    m = LlamaForCausalLM(cfg).eval()
    m.load_state_dict(sd, strict=True)
    for padding in ("right", "left"):
        x, am, pos = O.llama_inputs(lc, 5, 3, 13, padding)
        with torch.no_grad():
            ref = m(inputs_embeds=x, attention_mask=am, position_ids=pos).logits
        _, got = O.llama_forward(sd, lc, x, am, pos)
        assert torch.equal(got[am.bool()], ref[am.bool()])


def test_checkpoint_key_names_load_in_the_reference_and_back(tok, tmp_path):
    """A stage-1 checkpoint written by setok_amd.checkpoint loads in the reference's SetokTokenizer through the reference's own
    `get_w(weights, 'tokenizer')` + `load_state_dict(strict=False)` (setokim_arch.py:94-99), and a reference-side checkpoint loads here.
    The reference's side is its recorded state-dict layout (every key and shape: what load_state_dict(strict=False) matches and checks)
    and its head's values."""
    from setok_amd import SetokTokenizer, checkpoint as C
    torch.manual_seed(5)
    vc = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=3, num_attention_heads=4, image_size=112, patch_size=14)
    mine = SetokTokenizer(vision_tower=vc, hidden_dim=64, token_feat_dim=96, min_cluster_num=8, nheads=2, dim_feedforward=128)
    with torch.no_grad():
        for n, p in mine.named_parameters():
            if not n.startswith("image_feature_encoder."):
                p.copy_(torch.randn_like(p))
    path = tmp_path / "setok_stage1.bin"
    C.save_tokenizer_checkpoint(mine, path)

    weights = torch.load(path, map_location="cpu")
    get_w = lambda weights, keyword: {k.split(keyword + '.')[1]: v for k, v in weights.items() if keyword in k}      # as the reference spells it
    loaded = get_w(weights, "tokenizer")
    ref_keys = [str(k) for k in tok["ref_keys"]]
    unexpected_keys = [k for k in loaded if k not in ref_keys]
    missing_keys = [k for k in ref_keys if k not in loaded]
    assert unexpected_keys == []
    assert all(k.startswith("image_feature_encoder.") for k in missing_keys)
    assert all(tuple(v.shape) == tuple(int(d) for d in tok["shape:" + k]) for k, v in loaded.items())     # (a mismatch raises in load_state_dict)
    my_sd = mine.state_dict()
    head = [k for k in my_sd if not k.startswith("image_feature_encoder.")]
    assert len(head) >= 34 and all(torch.equal(loaded[k], my_sd[k]) for k in head)

    # the other direction: the stage-1 model's state dict holds the tokenizer under `tokenizer.` (and a detokenizer beside it)
    theirs = {"tokenizer." + k: _t(tok, "w:" + k) for k in ref_keys if not k.startswith("image_feature_encoder.")}
    theirs["detokenizer.decoder_norm.weight"] = torch.ones(3)             # comes along through the keyword match, dropped by strict=False
    res = C.load_pretrained_tokenizer(mine, theirs)
    assert res.unexpected_keys == ["decoder_norm.weight"]
    assert all(torch.equal(_t(tok, "w:" + k), mine.state_dict()[k]) for k in head)


def test_lm_loss_restatement_vs_reference_statements_live(tok):
    """The oracle's lm_loss against the recorded values of the reference's own loss statements, executed from the reference file
    (rac_harness.rac_lm_loss)."""
    for i, (seed, B, T, V, padding) in enumerate(((0, 2, 9, 37, "none"), (5, 4, 17, 101, "right"), (6, 3, 13, 64, "left"))):
        logits, labels, am = O.lm_loss_inputs(seed, B, T, V, padding)
        assert torch.equal(_t(tok, f"lm_loss:{i}"), O.lm_loss(logits, labels, am))


def test_pixel_terms_equal_the_reference_losses(tok):
    """§8(f) row 2: the oracle's pixel terms against the reference's own WeightedMSELoss module (loss/mse.py, loaded by file path; its
    output recorded) and the statements of the GAN loss's pixel term (loss/discriminator.py:161,170: torch.abs(inputs - reconstructions), torch.mean)."""
    g = torch.Generator().manual_seed(1)
    a, b = torch.randn(4, 3, 28, 42, generator=g), torch.randn(4, 3, 28, 42, generator=g)
    assert torch.equal(O.pixel_loss(a, b, "mse"), _t(tok, "pixel_mse"))
    assert torch.equal(O.pixel_loss(a, b, "l1"), torch.mean(torch.abs(b.contiguous() - a.contiguous())))


def test_stage2_oracle_projector_and_splice_match_the_reference_autograd(tok):
    """The stage-2 golden (tests/golden/stage2.npz) is generated by rac_stage2_grads; here the same quantities come from the ORACLE's projector +
    splice under torch autograd, against what the reference's modules gave (its projector's seeded parameters, loss, embeddings, labels and
    gradients, recorded): equal loss and gradients (fp32 rounding)."""
    seed, B, T, V, Dt, Dh = 21, 4, 11, 30, 48, 32
    ids, am, labels, feats, W = O.splice_inputs(seed, B, T, V, Dh)
    g = torch.Generator().manual_seed(seed)
    toks = [torch.randn(f.shape[0], Dt, generator=g) for f in feats]
    w_down = torch.randn(V, Dh, generator=g) * 0.3
    pos = torch.arange(T).expand(B, T).clone()
    loss, embeds, new_labels = _t(tok, "stage2:loss"), _t(tok, "stage2:embeds"), _t(tok, "stage2:new_labels")
    pg = {k[len("stage2:grad:"):]: _t(tok, k) for k in tok.files if k.startswith("stage2:grad:")}
    tg = [_t(tok, f"stage2:tokens_grad:{i}") for i in range(len(toks))]
    psd = {k[len("stage2:param:"):]: _t(tok, k).requires_grad_(True) for k in tok.files if k.startswith("stage2:param:")}
    assert len(pg) == len(psd) > 0
    tl = [t.clone().requires_grad_(True) for t in toks]
    of = [O.projector_forward(psd, "mlp2x_gelu", t) for t in tl]
    _, _, oemb, olab = O.splice_multimodal(ids, pos, am, labels, of, W)
    ol = O.stage2_downstream(oemb, olab, w_down)
    ol.backward()
    assert torch.equal(olab, new_labels) and torch.allclose(oemb, embeds, rtol=1e-6, atol=1e-6) and torch.allclose(ol, loss, rtol=1e-6)
    for n in pg:
        assert torch.allclose(psd[n].grad, pg[n], rtol=1e-4, atol=1e-6), n
    for a, b in zip(tl, tg):
        assert torch.allclose(a.grad if a.grad is not None else torch.zeros_like(a), b, rtol=1e-4, atol=1e-6)
