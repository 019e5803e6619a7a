"""The splice programs (tests/splice_cases.py) on the CPU: every program has the features it promises, the plain-Python restatement of the device
plan equals the CPU oracle on every program, truncation and padding side, every slip of the restatement is caught by a program, and the oracle
equals the reference's own recorded outputs (tests/golden/splice_programs.npz).  tests/test_splice_programs_gpu.py holds the kernels to the same
oracle and the same restatement."""
import functools
import os

import numpy as np
import pytest
import torch

import golden_io
import setok_oracle as O
import splice_cases as C

FIELDS = ("src", "labels", "mask", "position_ids")

# slip -> the programs on which the restatement with that slip differs from the oracle (some truncation, some side)
CATCHES = {
    "no_chunk_carry": ["chunk_edges", "crowded", "holes", "left_mask"],
    "no_image_carry": ["chunk_edges", "crowded", "holes", "left_mask"],
    "masked_placeholder_counts": ["holes", "left_mask", "nothing_kept"],
    "no_index_for_imageless": ["holes", "left_mask", "many_sequences"],
    "thread_prefix": ["many_sequences"],
    "trunc_whole_image": ["chunk_edges", "crowded", "holes", "left_mask", "many_sequences"],
    "target_kept": ["chunk_edges", "crowded", "holes", "left_mask", "many_sequences"],
}


@functools.lru_cache(maxsize=None)
def _oracle(name, trunc, side):
    ids, am, labels, lengths, _ = C.program(name)
    return C.oracle_plan(ids, am, labels, lengths, C.truncations(name)[trunc], side == "left")[0]


def _same(a, b):
    return all(getattr(a, f).shape == getattr(b, f).shape and torch.equal(getattr(a, f), getattr(b, f)) for f in FIELDS)


def _kept_placeholders(ids, am):
    return (ids == C.IMG) & (am != 0)


# ---- the programs hold what they promise --------------------------------------------------------------------------------------------------------
def test_every_program_is_seeded_small_table_and_has_enough_images():
    for name in C.PROGRAMS:
        ids, am, labels, lengths, v = C.program(name)
        again = C.BUILDERS[name]()
        assert all(torch.equal(x, y) for x, y in zip((ids, am, labels), again[:3])) and lengths == again[3], name
        assert v == C.V == 11 and ids.shape == am.shape == labels.shape
        text = ids[ids != C.IMG]
        assert int(text.min()) >= 0 and int(text.max()) < v
        spare = 2 if name in ("holes", "left_mask") else 0
        assert len(lengths) == C.images_needed(ids, am) + spare, name
        assert bool((labels[am == 0] == C.IGNORE).all())
        if name != "nothing_kept":
            assert bool(((labels == C.TARGET) & (am != 0) & (ids != C.IMG)).any()), name       # a TARGET label on a kept text token
            assert bool(((labels >= 0) & _kept_placeholders(ids, am)).any()), name             # a placeholder whose own label must not survive


def test_chunk_edges_features():
    ids, am, labels, lengths, _ = C.program("chunk_edges")
    assert ids.shape == (4, 513)                                                       # the third chunk holds one token
    where = [torch.nonzero(_kept_placeholders(ids, am)[b]).flatten().tolist() for b in range(4)]
    assert where == [[0, 255, 256, 257, 511, 512], [254, 255, 256], [300], [512]]
    assert {0, 1, 300} <= set(lengths) and max(lengths) > C.CHUNK
    assert not bool(((ids == C.IMG) & (am == 0)).any())
    plan, b, (p0, p1) = C.layout("chunk_edges")
    assert b == 0 and p1 - p0 == 300
    assert len(set(plan.seq_len.tolist())) == 4                                        # both padding sides pad


def test_crowded_features():
    ids, am, labels, lengths, _ = C.program("crowded")
    assert ids.shape == (3, 300)
    kept = _kept_placeholders(ids, am)
    assert kept.sum(1).tolist() == [46, 46, 46]
    for b in range(3):
        run = best = 0
        for f in kept[b].tolist():
            run = run + 1 if f else 0
            best = max(best, run)
        assert best >= 6
        assert int(kept[b, :C.CHUNK].sum()) > 30                                        # many in one chunk
    assert int(kept[0, C.CHUNK:].sum()) >= 1 and int(kept[1, C.CHUNK:].sum()) >= 1      # and some behind the carry
    assert set(lengths) == set(range(10))


@pytest.mark.parametrize("name", ["holes", "left_mask"])
def test_masked_programs_features(name):
    ids, am, labels, lengths, _ = C.program(name)
    assert ids.shape == (6, 300)
    kept = _kept_placeholders(ids, am)
    masked = (ids == C.IMG) & (am == 0)
    assert int(masked[:3].sum()) >= 1                                                   # placeholders under a zero mask bit, which consume nothing
    assert int(am[3].sum()) == 0 and int(masked[3].sum()) >= 1                          # nothing kept
    assert int(am[4].sum()) == 1 and int(kept[4].sum()) == 1                            # only a placeholder
    assert int(am[5].sum()) > 100 and int(kept[5].sum()) == 0 and int(masked[5].sum()) >= 1
    for b in range(3):
        assert int(kept[b].sum()) >= 3
        frac = float(am[b].float().mean())
        d = am[b, 1:] - am[b, :-1]
        if name == "holes":
            assert 0.7 < frac < 0.9 and int((d != 0).sum()) > 50                        # holes, not a prefix
        else:
            assert 0.5 <= frac <= 1.0 and bool((d >= 0).all()) and int(am[b, -1]) == 1  # left-padded
    if name == "left_mask":
        assert len({int(am[b].sum()) for b in range(3)}) == 3
    plan = C.layout(name)[0]
    used = -(plan.src[(plan.src < 0) & (plan.src != C.PAD)].long() + 1)
    assert int(used.max()) < sum(lengths[:-2]) and lengths[-1] > 0 and lengths[-2] > 0  # the two spare images are never read


def test_many_sequences_features():
    ids, am, labels, lengths, _ = C.program("many_sequences")
    B, T = ids.shape
    assert (B, T) == (515, 20) and B > 2 * C.CHUNK
    per = (B + C.CHUNK - 1) // C.CHUNK
    assert per == 3 and (C.CHUNK - 1) * per >= B                                        # the last threads own nothing
    assert bool((am[:, 1:] <= am[:, :-1]).all()) and int(am.sum(1).min()) >= 1          # prefix masks
    n = _kept_placeholders(ids, am).sum(1)
    assert sorted(set(n.tolist())) == [0, 1, 2, 3]
    for r in range(per):                                                               # a sequence without a placeholder in every slot of a thread
        assert bool((n[r::per] == 0).any())
    assert set(lengths) == {1, 2, 3, 4, 5}
    assert not bool(((ids == C.IMG) & (am == 0)).any())


def test_nothing_kept_features():
    ids, am, labels, lengths, _ = C.program("nothing_kept")
    assert ids.shape == (3, 9) and int(am.sum()) == 0 and bool((ids == C.IMG).any())
    for side in C.SIDES:
        plan = _oracle("nothing_kept", "above", side)
        assert plan.src.shape == (3, 0)


@pytest.mark.parametrize("name", [n for n in C.PROGRAMS if n != "nothing_kept"])
def test_truncations_land_where_they_say(name):
    """Judged on the ORACLE's untruncated layout: `max_length = L` keeps positions < L of every sequence."""
    ids, am, labels, lengths, _ = C.program(name)
    full = _oracle(name, "above", "right")
    tr = C.truncations(name)
    assert list(tr) == C.TRUNCS
    lens = full.mask.sum(1)
    b = int(lens.argmax())
    assert tr["above"] > int(lens.max()) and tr["one"] == 1
    row = full.src[b].tolist()
    off = C.offsets(lengths)

    def image_of(p):
        s = row[p]
        if s >= 0 or s == C.PAD:
            return None
        r = -(s + 1)
        return next(i for i in range(len(lengths)) if off[i] <= r < off[i + 1])

    i = image_of(tr["first_row"] - 1)
    assert i is not None and lengths[i] >= 3
    assert image_of(tr["first_row"] - 2) != i and image_of(tr["first_row"]) == i         # the last kept row is the image's first
    m = tr["middle_row"]
    assert tr["first_row"] < m < tr["last_row"] and image_of(m - 1) == i and image_of(m) == i
    assert image_of(tr["last_row"] - 1) == i and image_of(tr["last_row"]) != i           # ... its last
    assert tr["after"] == tr["last_row"] + 1 <= int(lens[b])
    assert row[tr["text"] - 1] >= 0 and tr["text"] > 2                                  # the last kept row is a text token
    for key in ("first_row", "middle_row", "last_row", "after"):                        # the cut shortens one sequence and leaves another whole:
        assert int((lens > tr[key]).sum()) >= 1 and int((lens < tr[key]).sum()) >= 1, key  # there are rows to pad, on either side
    if name == "chunk_edges":                                                           # the cut at T > 256: inside the image whose placeholder opens chunk 1
        assert lengths[i] == 300 and tr["middle_row"] > C.CHUNK


# ---- the restatement is the oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.PROGRAMS)
def test_plan_emulate_equals_the_oracle(name):
    ids, am, labels, lengths, _ = C.program(name)
    for trunc, ml in C.truncations(name).items():
        for side in C.SIDES:
            ref = _oracle(name, trunc, side)
            emu = C.plan_emulate(ids, am, labels, lengths, ml, side == "left")
            for f in FIELDS:
                assert torch.equal(getattr(emu, f), getattr(ref, f)), (name, trunc, side, f)
            assert emu.src.dtype == torch.int32
            assert emu.seq_len.tolist() == ref.mask.sum(1).tolist()


def test_plan_emulate_without_mask_and_labels():
    ids, am, labels, lengths, _ = C.unmasked("holes")
    assert am is None and labels is None and len(lengths) > len(C.program("holes")[3])
    ref, _ = C.oracle_plan(ids, None, None, lengths, 70, True)
    emu = C.plan_emulate(ids, None, None, lengths, 70, True)
    assert emu.labels is None and ref.labels is None
    assert torch.equal(emu.src, ref.src) and torch.equal(emu.position_ids, ref.position_ids) and torch.equal(emu.mask, ref.mask)


@pytest.mark.parametrize("slip", C.SLIPS)
def test_every_slip_is_caught(slip):
    caught = []
    for name in C.PROGRAMS:
        ids, am, labels, lengths, _ = C.program(name)
        hit = False
        for trunc, ml in C.truncations(name).items():
            for side in C.SIDES:
                hit = hit or not _same(C.plan_emulate(ids, am, labels, lengths, ml, side == "left", slip=slip), _oracle(name, trunc, side))
        if hit:
            caught.append(name)
    print(slip, "caught by", caught)
    assert caught, f"no program catches {slip}"
    assert caught == CATCHES[slip]


def test_truncating_slip_is_caught_by_the_truncations_inside_an_image():
    """`trunc_whole_image` must show on the cuts inside an image and only there."""
    ids, am, labels, lengths, _ = C.program("chunk_edges")
    full = _oracle("chunk_edges", "above", "right")
    off = torch.tensor(C.offsets(lengths))
    inside = []
    for trunc, ml in C.truncations("chunk_edges").items():
        splits = False
        for b in range(ids.shape[0]):
            if ml < int(full.mask[b].sum()):
                s0, s1 = int(full.src[b, ml - 1]), int(full.src[b, ml])
                splits = splits or (s0 < 0 and s1 < 0 and int(torch.searchsorted(off, -s0 - 1, right=True)) == int(torch.searchsorted(off, -s1 - 1, right=True)))
        if splits:
            inside.append(trunc)
        for side in C.SIDES:
            same = _same(C.plan_emulate(ids, am, labels, lengths, ml, side == "left", slip="trunc_whole_image"), _oracle("chunk_edges", trunc, side))
            assert same == (not splits), (trunc, side)
    assert inside == ["first_row", "middle_row", "one"]                                 # (sequence 0 opens with a 3-row image)


# ---- the oracle is the reference ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.RECORDED_PROGRAMS)
def test_oracle_equals_the_reference_recordings(golden_dir, name):
    z = golden_io.load(os.path.join(golden_dir, "splice_programs.npz"))
    for case in C.RECORDED:
        ids, am, labels, lengths, max_length, left = C.recorded_case(name, case)
        B, T = ids.shape
        key = f"{name}:{case}"
        assert [int(v) for v in z[key + ":spec"]] == [B, T, len(lengths), sum(lengths), -1 if max_length is None else max_length, 1 if left else 0]
        W, packed = C.tables(lengths, C.F32)
        pos = None if case == "none" else torch.arange(T).expand(B, T).clone()
        p, a, e, l = O.splice_multimodal(ids, pos, am, labels, C.split(packed, lengths), W, max_length=max_length,
                                         padding_side="left" if left else "right")
        rec = torch.from_numpy(np.asarray(z[key + ":embeds"]))
        assert e.dtype == rec.dtype == torch.float32 and torch.equal(e, rec), key
        if case == "none":
            assert p is None and a is None and l is None and key + ":pos" not in z
        else:
            for got, k in ((p, "pos"), (a, "mask"), (l, "labels")):
                rec = torch.from_numpy(np.asarray(z[f"{key}:{k}"]))
                assert got.dtype == rec.dtype and torch.equal(got, rec), (key, k)
        # the value-table helper reads the same rows: its fp32 columns are these tables
        if case != "none":
            rows = C.oracle_run(ids, am, labels, lengths, max_length, left)[2]
            assert torch.equal(C.embeds_of(rows, C.F32), e)
