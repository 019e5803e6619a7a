"""The multimodal splice (setok_amd/csrc/splice.hip) on a real MI355X under the programs of tests/splice_cases.py: placeholders on the edges of the
plan kernel's 256-token chunks, an image longer than a chunk and one without rows, masks with holes and left-padded masks, B = 515 (three sequences
per thread of the lengths kernel), the truncation on the first / a middle / the last row of an image, real row widths with guard rows around the
output, the zero-fill `status` path, the first-bad-id report, and the backward scatter with repeated ids.  The yardsticks are the CPU oracle
(oracle/setok_oracle.py: splice_multimodal, held to the reference's own recorded outputs by tests/test_splice_programs_cpu.py) and the plain-Python
restatement of the device plan that the same file holds equal to the oracle.  Integers and row copies: everything is compared bit for bit, except
d embed_tokens.weight, whose fp32 atomics fix no summation order (bound below).  `pytest -m gpu`."""
import functools
import os

import pytest
import torch

import setok_oracle as O
import splice_cases as C

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import setok_amd
    from setok_amd import _lib, ops
    from setok_amd.tokenizer import RaggedTokens

DEV = "cuda"
F32, BF16, F16 = C.F32, C.BF16, C.F16
INT_VIEW = {F32: torch.int32, BF16: torch.int16, F16: torch.int16}
ES = {F32: 4, BF16: 2, F16: 2}
IMG_INDEX, IGNORE_INDEX, TARGET_INDEX = C.IMG, C.IGNORE, C.TARGET


def _bits_equal(got, ref):
    """Same shape, same dtype, same bytes (-0.0 and NaN payloads included)."""
    got = got.detach().cpu()
    return got.shape == ref.shape and got.dtype == ref.dtype and torch.equal(got.contiguous().view(INT_VIEW[ref.dtype]), ref.contiguous().view(INT_VIEW[ref.dtype]))


def _log(what, value, bound):
    path = os.environ.get("SETOK_PARITY_LOG")
    if path:
        test = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]
        with open(path, "a") as f:
            f.write(f"{test}\t{what}\t{value:.3e}\tbound {bound:.3e}\n")
    print(what, f"{value:.3e}", f"bound {bound:.3e}")


def _ragged(packed, lengths):
    return RaggedTokens(packed.to(DEV), lengths)


def _device_offsets(lengths):
    return torch.tensor(C.offsets(lengths), dtype=torch.int32, device=DEV)


# ---- plan and rows against the oracle, through the wrapper ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,trunc,side", C.cases(), ids=lambda v: str(v))
def test_splice_multimodal_equals_the_oracle(name, trunc, side):
    """One oracle call per case: its fp64 rows carry fp32, bf16 and fp16 columns (splice_cases.value_tables).  The caller's dtypes are kept: a bool
    mask on the middle-row cuts, int32 position ids on the left-padded cases."""
    ids, am, labels, lengths, _ = C.program(name)
    ml, left = C.truncations(name)[trunc], side == "left"
    am = am.bool() if trunc in ("middle_row", "one") else am
    pos_dtype = torch.int32 if left else torch.int64
    B, T = ids.shape
    pos = torch.arange(T, dtype=pos_dtype).expand(B, T).clone()
    rp, ra, rows, rl = C.oracle_run(ids, am, labels, lengths, ml, left, pos_dtype=pos_dtype)
    assert rp.dtype == pos_dtype and ra.dtype == am.dtype
    if name == "nothing_kept":
        assert rows.shape == (B, 0, C.N_COLS)
    for dt in C.DTS:
        W, packed = C.tables(lengths, dt)
        p, a, e, l = setok_amd.splice_multimodal(ids.to(DEV), pos.to(DEV), am.to(DEV), labels.to(DEV), _ragged(packed, lengths), W.to(DEV),
                                                 max_length=ml, padding_side=side)
        assert _bits_equal(e, C.embeds_of(rows, dt)), (C.NAME[dt], "inputs_embeds")
        for got, ref, what in ((p, rp, "position_ids"), (a, ra, "attention_mask"), (l, rl, "labels")):
            assert got.dtype == ref.dtype and got.shape == ref.shape and torch.equal(got.cpu(), ref), (C.NAME[dt], what)


@pytest.mark.parametrize("dt,name,trunc,side", [(F32, "chunk_edges", "above", "right"), (BF16, "crowded", "middle_row", "left"),
                                                (F16, "holes", "text", "right")], ids=lambda v: C.NAME.get(v, str(v)))
def test_none_conventions(dt, name, trunc, side):
    """setokim_arch.py:341-353: an optional input that is None comes back None; without a mask every token is kept (the placeholders a zero mask
    bit used to hide then consume images of their own: splice_cases.unmasked)."""
    ids, am, labels, lengths, _ = C.program(name)
    _, _, _, lengths_all, _ = C.unmasked(name)
    ml, left = C.truncations(name)[trunc], side == "left"
    B, T = ids.shape
    pos = torch.arange(T).expand(B, T).clone()
    variants = {"no_position_ids": (None, am, labels, lengths), "no_labels": (pos, am, None, lengths), "no_mask": (pos, None, labels, lengths_all),
                "none": (None, None, None, lengths_all)}
    for what, (p_, a_, l_, lens) in variants.items():
        W64, F64 = C.value_tables(sum(lens), 7)
        rp, ra, rows, rl = O.splice_multimodal(ids, p_, a_, l_, C.split(F64, lens), W64, max_length=ml, padding_side=side)
        W, packed = C.tables(lens, dt)
        dev = lambda t: None if t is None else t.to(DEV)
        p, a, e, l = setok_amd.splice_multimodal(ids.to(DEV), dev(p_), dev(a_), dev(l_), _ragged(packed, lens), W.to(DEV), max_length=ml, padding_side=side)
        assert _bits_equal(e, C.embeds_of(rows, dt)), what
        for got, ref, field in ((p, rp, "position_ids"), (a, ra, "attention_mask"), (l, rl, "labels")):
            if ref is None:
                assert got is None, (what, field)
            else:
                assert got.dtype == ref.dtype and torch.equal(got.cpu(), ref), (what, field)
        assert (p is None) == (p_ is None) and (a is None) == (a_ is None) and (l is None) == (l_ is None)


@pytest.mark.parametrize("dt,name,trunc,side", [(F32, "crowded", "middle_row", "left"), (BF16, "holes", "above", "right"),
                                                (F16, "many_sequences", "first_row", "left")], ids=lambda v: C.NAME.get(v, str(v)))
def test_image_token_input_forms_give_the_same_bytes(dt, name, trunc, side):
    """RaggedTokens, a list of (L_i, D) tensors and a dense (n, L, D) tensor, on the program with every image 3 rows long."""
    L = 3
    ids, am, labels, lengths, _ = C.uniform_lengths(name, L)
    ml, left = C.truncations(name)[trunc], side == "left"
    rp, ra, rows, rl = C.oracle_run(ids, am, labels, lengths, ml, left)
    W, packed = C.tables(lengths, dt)
    forms = {"ragged": _ragged(packed, lengths), "list": [f.to(DEV) for f in C.split(packed, lengths)],
             "dense": packed.reshape(len(lengths), L, -1).to(DEV)}
    for what, feats in forms.items():
        p, a, e, l = setok_amd.splice_multimodal(ids.to(DEV), None, am.to(DEV), labels.to(DEV), feats, W.to(DEV), max_length=ml, padding_side=side)
        assert _bits_equal(e, C.embeds_of(rows, dt)), what
        assert p is None and torch.equal(a.cpu(), ra) and torch.equal(l.cpu(), rl), what


# ---- src itself ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.PROGRAMS)
def test_lengths_and_plan_equal_the_restated_plan(name):
    """ops.splice_lengths + ops.splice_plan against splice_cases.plan_emulate on every truncation and side: seq_len, img_start, src (pad rows
    INT32_MIN), labels, mask and position ids."""
    ids, am, labels, lengths, _ = C.program(name)
    ids_d, am_d, lab_d, off_d = ids.to(DEV), am.to(torch.uint8).to(DEV), labels.to(DEV), _device_offsets(lengths)
    for trunc, ml in C.truncations(name).items():
        for side in C.SIDES:
            emu = C.plan_emulate(ids, am, labels, lengths, ml, side == "left")
            seq_len, img_start, status = ops.splice_lengths(ids_d, am_d, off_d, len(lengths), IMG_INDEX, ml, vocab=C.V)
            st = status.cpu().tolist()
            assert st[0] == 0 and st[1] == C.images_needed(ids, am) and st[2] == 0 and st[3] == -1, (trunc, side, st)
            assert torch.equal(seq_len.cpu(), emu.seq_len) and torch.equal(img_start.cpu(), emu.img_start), (trunc, side)
            max_len = int(emu.seq_len.max())
            src, nl, nm, npos = ops.splice_plan(ids_d, am_d, lab_d, off_d, seq_len, img_start, max_len, side == "left", IMG_INDEX, IGNORE_INDEX,
                                                TARGET_INDEX, want_mask=True, want_pos=True)
            assert src.shape == (ids.shape[0], max_len) and src.dtype == torch.int32
            if max_len == 0:
                continue
            assert torch.equal(src.cpu(), emu.src), (trunc, side)
            assert bool((src.cpu()[emu.mask == 0] == -(1 << 31)).all())
            assert torch.equal(nl.cpu(), emu.labels) and torch.equal(nm.cpu().long(), emu.mask) and torch.equal(npos.cpu(), emu.position_ids), (trunc, side)


# ---- rows at real widths ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _crowded_src():
    """src of `crowded` cut in the middle of an image and left-padded: ids, image rows and pad rows."""
    ids, am, labels, lengths, _ = C.program("crowded")
    src = C.plan_emulate(ids, am, labels, lengths, C.truncations("crowded")["middle_row"], True).src
    flat = src.reshape(-1)
    assert int((flat == C.PAD).sum()) > 0 and int((flat >= 0).sum()) > 0 and int(((flat < 0) & (flat != C.PAD)).sum()) > 0
    return src, sum(lengths)


def _expected_rows(src, W, packed):
    flat = src.reshape(-1).long()
    out = torch.zeros((flat.numel(), W.shape[1]), dtype=W.dtype)
    text, image = flat >= 0, (flat < 0) & (flat != C.PAD)
    out[text] = W[flat[text]]
    out[image] = packed[-(flat[image] + 1)]
    return out


def _random_tables(dt, D, n_rows, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(C.V, D, generator=g).to(dt), torch.randn(n_rows, D, generator=g).to(dt)


@pytest.mark.parametrize("dt,D", [(F32, 4), (F32, 12), (F32, 256), (F32, 260), (BF16, 8), (BF16, 520), (BF16, 4096), (F16, 8), (F16, 520), (F16, 4096)],
                         ids=lambda v: C.NAME.get(v, str(v)))
def test_rows_at_real_widths_with_guard_rows(dt, D):
    """Rows of 16, 48, 1024, 1040 and 8192 bytes (a wave moves 1024 bytes per pass) written into the middle of a NaN-filled buffer: image rows and
    embedding rows bit-equal, pad rows exactly zero, the guard rows in front and behind untouched."""
    src, n_rows = _crowded_src()
    W, packed = _random_tables(dt, D, n_rows, 11)
    rows, guard = src.numel(), 4
    buf = torch.full((guard + rows + guard, D), float("nan"), dtype=dt, device=DEV)
    src_d, W_d, packed_d = src.to(DEV), W.to(DEV), packed.to(DEV)
    assert (guard * D * ES[dt]) % 16 == 0
    _lib.call("setok_splice_rows", ops._stream(), ops._code(dt), src_d.data_ptr(), W_d.data_ptr(), C.V, packed_d.data_ptr(), n_rows,
              buf.data_ptr() + guard * D * ES[dt], rows, D, None)
    got = buf.cpu()
    assert bool(torch.isnan(got[:guard]).all()) and bool(torch.isnan(got[guard + rows:]).all())
    exp = _expected_rows(src, W, packed)
    assert _bits_equal(got[guard:guard + rows], exp)
    pad = src.reshape(-1) == C.PAD
    assert bool((got[guard:guard + rows][pad].view(INT_VIEW[dt]) == 0).all())


# ---- the status path -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", C.DTS, ids=lambda v: C.NAME[v])
def test_rows_neither_table_can_serve_are_zero_filled_and_reported(dt):
    """With the true `vocab` and `image_token_rows`: an id equal to vocab and an image row equal to image_token_rows are the first values past
    each table; by the kernel's own checks (s < vocab, fr < feat_rows) neither becomes an address."""
    src, n_rows = _crowded_src()
    D = 3 * C.WIDTH[dt]
    W, packed = _random_tables(dt, D, n_rows, 12)
    W_d, packed_d = W.to(DEV), packed.to(DEV)
    status = torch.full((2,), -5, dtype=torch.int32, device=DEV)
    clean = ops.splice_rows(src.to(DEV), W_d, packed_d, status)
    assert status.cpu().tolist()[0] == 0
    exp = _expected_rows(src, W, packed)
    assert _bits_equal(clean.reshape(-1, D), exp)
    bad_rows = {700: C.V, 301: -(n_rows + 1), 1000: C.V, 302: C.V}
    bad = src.clone().reshape(-1)
    for r, s in bad_rows.items():
        bad[r] = s
    got = ops.splice_rows(bad.reshape(src.shape).to(DEV), W_d, packed_d, status)
    assert status.cpu().tolist() == [1, min(bad_rows)]
    exp_bad = exp.clone()
    exp_bad[list(bad_rows)] = 0
    assert _bits_equal(got.reshape(-1, D), exp_bad)                       # those rows zero, every other row intact
    # no image tokens handed over: every image row is zero-filled, the first one reported; text rows intact
    got = ops.splice_rows(src.to(DEV), W_d, None, status)
    flat = src.reshape(-1)
    image = (flat < 0) & (flat != C.PAD)
    assert status.cpu().tolist() == [1, int(torch.nonzero(image)[0])]
    exp_none = exp.clone()
    exp_none[image] = 0
    assert _bits_equal(got.reshape(-1, D), exp_none)


# ---- errors through the wrapper ----------------------------------------------------------------------------------------------------------------
def _call(ids, am, labels, lengths, **kw):
    W, packed = C.tables(lengths, F32)
    return setok_amd.splice_multimodal(ids.to(DEV), None, am.to(DEV), labels.to(DEV), _ragged(packed, lengths), W.to(DEV), **kw)


def test_one_image_short_at_many_sequences_raises():
    ids, am, labels, lengths, _ = C.program("many_sequences")
    need = C.images_needed(ids, am)
    assert need == len(lengths)
    with pytest.raises(IndexError, match=rf"needs {need} images but only {need - 1}"):
        _call(ids, am, labels, lengths[:-1])


def test_first_bad_id_is_reported_across_chunks_and_threads():
    ids, am, labels, lengths, _ = C.program("chunk_edges")
    b = 1
    assert all(int(am[b, t]) == 1 and int(ids[b, t]) != C.IMG for t in (40, 300))
    one = ids.clone(); one[b, 300] = C.V                                  # a single bad id behind the first chunk
    with pytest.raises(IndexError, match=rf"input_ids\[{b}, 300\]"):
        _call(one, am, labels, lengths)
    two = ids.clone(); two[b, 300] = C.V + 3; two[b, 40] = -7             # two in one sequence: the earlier one, though a later thread finds it
    with pytest.raises(IndexError, match=rf"input_ids\[{b}, 40\]"):
        _call(two, am, labels, lengths)
    ids, am, labels, lengths, _ = C.program("many_sequences")
    ids, am = ids.clone(), am.clone()
    am[300, :8] = 1; am[400, :3] = 1                                      # (still prefix masks; both positions kept)
    ids[300, 7] = C.V; ids[400, 2] = C.TARGET
    lengths = lengths + [1, 1]                                            # (images to spare, whatever the two ids replaced)
    with pytest.raises(IndexError, match=r"input_ids\[300, 7\]"):
        _call(ids, am, labels, lengths)


def test_bad_id_under_a_zero_mask_bit_raises_nothing():
    ids, am, labels, lengths, _ = C.program("holes")
    hidden = torch.nonzero((am == 0) & (ids != C.IMG))
    assert hidden.numel() > 0
    bad = ids.clone()
    for b, t in hidden[:: max(1, len(hidden) // 7)].tolist():
        bad[b, t] = C.V if (b + t) % 2 else -7
    bad[3, 0] = C.V + 100                                                 # ... in the sequence with nothing kept as well
    _, ra, rows, rl = C.oracle_run(ids, am, labels, lengths, None, False)
    p, a, e, l = _call(bad, am, labels, lengths)
    assert _bits_equal(e, C.embeds_of(rows, F32)) and torch.equal(a.cpu(), ra) and torch.equal(l.cpu(), rl)


# ---- backward, direct --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bwd_src():
    """src of `holes` cut in the middle of an image and left-padded, with the ids renamed so that id 9 is carried by one row and id 10 by none
    (at V = 11 every id would repeat otherwise): repeated ids, a single one, an absent one, image rows kept and dropped, spare images, pad rows."""
    ids, am, labels, lengths, _ = C.program("holes")
    ml = C.truncations("holes")["middle_row"]
    ids = ids.clone()
    ids[ids == 10] = 4
    first = C.plan_emulate(ids, am, labels, lengths, ml, True).src
    once = torch.nonzero((ids == 9) & (am != 0))
    ids[ids == 9] = 3
    src = None
    for b, t in once.tolist():                                            # the first id 9 that survives the cut keeps its name
        trial = ids.clone(); trial[b, t] = 9
        src = C.plan_emulate(trial, am, labels, lengths, ml, True).src
        if int((src == 9).sum()) == 1:
            break
    assert src is not None and int((src == 9).sum()) == 1 and int((src == 10).sum()) == 0 and src.shape == first.shape
    return src, lengths


def _embed_grad_check(dem, src, d_out, label, ref64=None):
    """d embed[v] = sum of d_out rows whose src is v, accumulated by fp32 atomics in no fixed order.  Against the fp64 sum of the same rows, per
    element: |error| <= n * 2^-24 * sum |terms|, n the number of rows that carry v — recursive fp32 summation of n terms in ANY order is off by at
    most (n - 1) u sum|terms| to first order in u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2), and the terms
    themselves are exact (every dtype's value is an fp32 value).  n == 1: the fp32 cast itself; n == 0: zero.  `ref64`: the fp64 reference to
    judge against where the caller has one of its own (torch.autograd through the oracle), which must be that same sum up to fp64 rounding."""
    flat = src.reshape(-1).long()
    text = flat >= 0
    d64 = d_out.reshape(flat.numel(), -1).double().cpu()
    V, D = dem.shape
    ref = torch.zeros(V, D, dtype=torch.float64).index_add_(0, flat[text], d64[text])
    mag = torch.zeros(V, D, dtype=torch.float64).index_add_(0, flat[text], d64[text].abs())
    n = torch.bincount(flat[text], minlength=V).double()
    bound = n[:, None] * 2.0 ** -24 * mag
    if ref64 is not None:
        assert ref64.dtype == torch.float64 and bool(((ref64 - ref).abs() <= n[:, None] * 2.0 ** -53 * mag).all())
        ref = ref64
    got = dem.detach().cpu()
    assert got.dtype == torch.float32
    err = (got.double() - ref).abs()
    worst = int(torch.where(bound > 0, err / bound, err).argmax())         # the element that uses most of its bound
    _log(f"{label}: d_embed max |err|", float(err.max()), float(bound.reshape(-1)[int(err.argmax())]))
    _log(f"{label}: d_embed |err| nearest its bound", float(err.reshape(-1)[worst]), float(bound.reshape(-1)[worst]))
    assert bool((err <= bound).all()), (label, float(err.reshape(-1)[worst]), float(bound.reshape(-1)[worst]))
    single, absent = n == 1, n == 0
    assert torch.equal(got[single], ref[single].float())
    assert bool((got[absent].view(torch.int32) == 0).all())
    return n


def _image_grad_expected(src, d_out, n_rows):
    flat = src.reshape(-1).long()
    image = (flat < 0) & (flat != C.PAD)
    d = d_out.reshape(flat.numel(), -1).cpu()
    exp = torch.zeros((n_rows, d.shape[1]), dtype=d.dtype)
    fr = -(flat[image] + 1)
    assert fr.unique().numel() == fr.numel()                             # an image row is consumed by at most one output position
    exp[fr] = d[image]
    return exp, fr


@pytest.mark.parametrize("dt", C.DTS, ids=lambda v: C.NAME[v])
def test_rows_bwd_direct(dt):
    src, lengths = _bwd_src()
    n_rows = sum(lengths)
    D = 3 * C.WIDTH[dt]
    d_out = torch.randn(src.numel(), D, generator=torch.Generator().manual_seed(13)).to(dt)        # on the dtype's grid; pad rows carry values too
    src_d, d_out_d = src.to(DEV), d_out.to(DEV)
    exp, used = _image_grad_expected(src, d_out, n_rows)
    dropped = torch.ones(n_rows, dtype=torch.bool); dropped[used] = False
    spare = sum(lengths[:-2])
    assert int(dropped[:spare].sum()) > 0 and bool(dropped[spare:].all())  # rows the cut dropped, and the two spare images

    dfe, dem = ops.splice_rows_bwd(src_d, d_out_d, n_rows, want_embed=C.V)
    assert _bits_equal(dfe, exp)
    assert bool((dfe.cpu()[dropped].view(INT_VIEW[dt]) == 0).all())
    n = _embed_grad_check(dem, src, d_out, f"rows_bwd {C.NAME[dt]}")
    assert int(n[9]) == 1 and int(n[10]) == 0 and int(n[:9].min()) > 1     # repeated ids, one carried once, one never

    dfe, dem = ops.splice_rows_bwd(src_d, d_out_d, n_rows, want_embed=0)    # the projector-only form
    assert dem is None and _bits_equal(dfe, exp)
    dfe, dem = ops.splice_rows_bwd(src_d, d_out_d, 0, want_embed=C.V)       # the embedding-only form
    assert dfe is None
    _embed_grad_check(dem, src, d_out, f"rows_bwd {C.NAME[dt]} embed only")


# ---- backward, through autograd ------------------------------------------------------------------------------------------------------------------
@pytest.mark.grad
def test_nothing_kept_under_autograd_gives_zero_gradients():
    """Width 0 forward (the outputs are empty buffers, whose addresses are null) and backward: every gradient is exactly zero."""
    ids, am, labels, lengths, _ = C.program("nothing_kept")
    W, packed = C.tables(lengths, F32)
    Wd, pd = W.clone().to(DEV).requires_grad_(True), packed.clone().to(DEV).requires_grad_(True)
    p, a, e, l = setok_amd.splice_multimodal(ids.to(DEV), None, am.to(DEV), labels.to(DEV), RaggedTokens(pd, lengths), Wd)
    assert e.shape == (3, 0, C.WIDTH[F32]) and a.shape == (3, 0) and l.shape == (3, 0) and e.grad_fn is not None
    e.sum().backward()
    for leaf in (Wd, pd):
        assert leaf.grad.shape == leaf.shape and bool((leaf.grad.cpu().view(torch.int32) == 0).all())


@pytest.mark.grad
def test_autograd_through_the_splice_equals_autograd_through_the_oracle():
    """`chunk_edges` cut inside its 300-row image, left-padded, fp32: gradients of sum(inputs_embeds * G) with respect to the packed image tokens
    (bit-equal: copies) and the embedding table (the atomics' bound) against torch.autograd through the oracle on the same leaves in fp64."""
    name, dt = "chunk_edges", F32
    ids, am, labels, lengths, _ = C.program(name)
    ml = C.truncations(name)["middle_row"]
    W, packed = C.tables(lengths, dt)
    Wd, pd = W.clone().to(DEV).requires_grad_(True), packed.clone().to(DEV).requires_grad_(True)
    p, a, e, l = setok_amd.splice_multimodal(ids.to(DEV), None, am.to(DEV), labels.to(DEV), RaggedTokens(pd, lengths), Wd, max_length=ml, padding_side="left")
    assert e.grad_fn is not None and e.shape[1] == ml
    G = torch.randn(e.shape, generator=torch.Generator().manual_seed(14))
    (e * G.to(DEV)).sum().backward()

    W64, p64 = W.double().requires_grad_(True), packed.double().requires_grad_(True)
    _, ra, re, rl = O.splice_multimodal(ids, None, am, labels, C.split(p64, lengths), W64, max_length=ml, padding_side="left")
    assert torch.equal(e.detach().cpu().double(), re.detach()) and torch.equal(a.cpu(), ra) and torch.equal(l.cpu(), rl)
    (re * G.double()).sum().backward()

    assert pd.grad.dtype == dt and _bits_equal(pd.grad, p64.grad.to(dt))
    off = C.offsets(lengths)
    assert bool((pd.grad.cpu()[off[2] + 151:off[3]] == 0).all()) and bool((pd.grad.cpu()[off[2]:off[2] + 151] != 0).any())   # the 300-row image: 151 rows kept
    src = C.plan_emulate(ids, am, labels, lengths, ml, True).src
    assert Wd.grad.dtype == dt
    _embed_grad_check(Wd.grad, src, G, "autograd chunk_edges fp32", ref64=W64.grad)
