"""Programs for the multimodal splice (setok_amd/csrc/splice.hip: setok_splice_lengths / _plan / _rows / _rows_bwd): seeded inputs that put
placeholders, mask holes and the truncation where the kernels change path, a plain-Python restatement of the device plan, and the slips — the
restatement wrong in one way such a kernel can be wrong.  Pure torch on the CPU; imports nothing of the library.

Every builder returns `(ids, attention_mask, labels, image_lengths, V)` with a small table (V = 11) so that ids repeat.  What each program is for:

  chunk_edges     B = 4, T = 513: the plan kernel walks a sequence in chunks of 256 tokens and carries the image count and the output position
                  between them; placeholders sit on both sides of every chunk edge, one image has 300 rows (longer than a chunk), one has none
  crowded         B = 3, T = 300: 46 placeholders per sequence (a run of six among them), image lengths 0..9: the two scans inside a chunk
  holes           B = 6, T = 300: a mask with holes, placeholders under zero mask bits, a sequence with nothing kept, one that keeps a single
                  placeholder, one whose placeholders are all masked; two spare images behind the consumed ones
  left_mask       the same with left-padded masks (batched generation)
  many_sequences  B = 515, T = 20: the lengths kernel gives each of its 256 threads ceil(B / 256) = 3 sequences and carries the image index
                  inside a thread; the last threads own nothing
  nothing_kept    B = 3, T = 9, mask all zero: the padded width is 0

`truncations(name)` derives the `max_length` values from the program's own untruncated layout (the cut on the first, a middle and the last row of
the longest image of the longest sequence, one position later, in text, 1, and above every length).

`plan_emulate` follows the kernels' structure (per-thread blocks of sequences for the image index, 256-token chunks with carries, max(n_img, 1),
truncation by row, the left shift); `oracle_plan` reads the same plan out of the CPU oracle (oracle/setok_oracle.py: splice_multimodal) by running
it on tables whose first column names the row.  tests/test_splice_programs_cpu.py holds the two equal and shows that every slip is caught."""
import collections
import functools

import torch

import setok_oracle as O

V = 11
IMG, IGNORE, TARGET = O.IMAGE_TOKEN_INDEX, O.IGNORE_INDEX, O.TARGET_TOKEN_INDEX
PAD = -(1 << 31)                                   # src of a zero row (SRC_PAD of splice.hip)
CHUNK = 256                                        # tokens per pass of the plan kernel = threads of the lengths kernel
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTS = [F32, BF16, F16]
NAME = {F32: "fp32", BF16: "bf16", F16: "fp16"}
WIDTH = {F32: 4, BF16: 8, F16: 8}                  # the narrowest rows the kernels take: 16 bytes
SLIPS = ["no_chunk_carry", "no_image_carry", "masked_placeholder_counts", "no_index_for_imageless", "thread_prefix", "trunc_whole_image",
         "target_kept"]
SIDES = ["right", "left"]
TRUNCS = ["first_row", "middle_row", "last_row", "after", "text", "one", "above"]

Plan = collections.namedtuple("Plan", "src labels mask position_ids seq_len img_start")


# ---- the programs ----------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ids(B, T, g):
    return torch.randint(0, V, (B, T), generator=g)


def _labels(am, g):
    """Random labels (a placeholder's own label must not survive), about 6 % TARGET_TOKEN_INDEX, IGNORE_INDEX under a zero mask bit."""
    B, T = am.shape
    lab = torch.randint(0, V, (B, T), generator=g)
    lab[torch.rand(B, T, generator=g) < 0.06] = TARGET
    lab[am == 0] = IGNORE
    return lab


def images_needed(ids, am):
    """Every kept placeholder consumes an image, and so does every sequence without one."""
    kept = ((ids == IMG) & (am != 0)).sum(1)
    return int(kept.clamp_min(1).sum())


def _rand_lengths(n, lo, hi, g):
    return [int(v) for v in torch.randint(lo, hi + 1, (n,), generator=g)]


def chunk_edges():
    B, T = 4, 513
    g = _gen(101)
    ids, am = _ids(B, T, g), torch.ones(B, T, dtype=torch.long)
    ids[0, [0, 255, 256, 257, 511, 512]] = IMG
    ids[1, 254:257] = IMG
    ids[2, 300] = IMG
    ids[3, 512] = IMG
    am[2, 350:] = 0                                # a prefix mask and a left-padded one: lengths differ, so both padding sides pad
    am[3, :400] = 0
    lengths = [3, 0, 300, 1, 5, 2] + [2, 0, 4] + [7] + [1]
    return ids, am, _labels(am, g), lengths, V


def crowded():
    B, T = 3, 300
    g = _gen(102)
    ids, am = _ids(B, T, g), torch.ones(B, T, dtype=torch.long)
    am[1, 280:] = 0
    am[2, 200:] = 0                                # (a shorter sequence: a cut late in the longest one still leaves rows to pad)
    for b in range(B):
        n = int(am[b].sum())
        run = int(torch.randint(0, n - 6, (1,), generator=g))
        ids[b, run:run + 6] = IMG
        rest = torch.tensor([t for t in range(n) if not run <= t < run + 6])
        ids[b, rest[torch.randperm(rest.numel(), generator=g)[:40]]] = IMG
    return ids, am, _labels(am, g), _rand_lengths(images_needed(ids, am), 0, 9, g), V


def _masked_program(seed, left):
    B, T = 6, 300
    g = _gen(seed)
    ids = _ids(B, T, g)
    ids[torch.rand(B, T, generator=g) < 0.04] = IMG
    if left:
        am = torch.zeros(B, T, dtype=torch.long)
        for b in range(B):
            am[b, T - int(torch.randint(150, T + 1, (1,), generator=g)):] = 1
    else:
        am = (torch.rand(B, T, generator=g) < 0.8).long()
    am[3] = 0                                      # nothing kept (its placeholders are all masked)
    am[4] = 0                                      # keeps a single placeholder
    t4 = T - 1 if left else 137
    ids[4, t4] = IMG; am[4, t4] = 1
    if left:                                       # keeps no placeholder but has masked ones
        kept5 = am[5] != 0
        ids[5, kept5 & (ids[5] == IMG)] = 3
        ids[5, 5] = IMG
        assert am[5, 5] == 0
    else:
        ids[5, 17] = IMG
        am[5, ids[5] == IMG] = 0
    lengths = _rand_lengths(images_needed(ids, am) + 2, 1, 12, g)         # two spare images behind the consumed ones
    return ids, am, _labels(am, g), lengths, V


def holes():
    return _masked_program(103, left=False)


def left_mask():
    return _masked_program(104, left=True)


def many_sequences():
    B, T = 515, 20
    g = _gen(105)
    ids, am = _ids(B, T, g), torch.zeros(B, T, dtype=torch.long)
    for b in range(B):
        n = int(torch.randint(1, T + 1, (1,), generator=g))
        am[b, :n] = 1
        k = min(int(torch.randint(0, 4, (1,), generator=g)), n)
        ids[b, torch.randperm(n, generator=g)[:k]] = IMG
    return ids, am, _labels(am, g), _rand_lengths(images_needed(ids, am), 1, 5, g), V


def nothing_kept():
    B, T = 3, 9
    g = _gen(106)
    ids, am = _ids(B, T, g), torch.zeros(B, T, dtype=torch.long)
    ids[1, 4] = IMG
    return ids, am, _labels(am, g), [2, 3, 1], V


BUILDERS = dict(chunk_edges=chunk_edges, crowded=crowded, holes=holes, left_mask=left_mask, many_sequences=many_sequences,
                nothing_kept=nothing_kept)
PROGRAMS = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def program(name):
    """The program's tensors, built once: callers that change one clone it first."""
    return BUILDERS[name]()


def uniform_lengths(name, L):
    """The program with every image L rows long: what the dense (n_images, L, D) input form can express."""
    ids, am, labels, lengths, v = program(name)
    return ids, am, labels, [L] * len(lengths), v


def unmasked(name):
    """The program for a call without a mask (and without labels): every token is kept, the placeholders a zero mask bit used to hide
    included, so further images (1, 2, 3, 1, ... rows) follow the program's own."""
    ids, am, labels, lengths, v = program(name)
    more = images_needed(ids, torch.ones_like(am)) - len(lengths)
    return ids, None, None, list(lengths) + [1 + i % 3 for i in range(max(more, 0))], v


def offsets(lengths):
    off = [0]
    for n in lengths:
        off.append(off[-1] + int(n))
    return off


# ---- the device plan, restated ---------------------------------------------------------------------------------------------------------------
def plan_emulate(ids, mask, labels, image_lengths, max_length, left, slip=None):
    """What setok_splice_lengths + setok_splice_plan compute, in their order of work.  `mask` / `labels` may be None as in the wrapper.  Returns
    Plan(src, labels, mask, position_ids, seq_len, img_start): src int32 (B, max_len) with >= 0 an id, < 0 packed image row -(r + 1), PAD a zero row.
    `slip` names one mistake (SLIPS)."""
    assert slip is None or slip in SLIPS, slip
    B, T = ids.shape
    idl = ids.tolist()
    keep = [[True] * T for _ in range(B)] if mask is None else (mask != 0).tolist()
    lab = None if labels is None else labels.tolist()
    off = offsets(image_lengths)
    n_images = len(image_lengths)
    # splice_count_kernel: kept tokens and kept placeholders per sequence
    n_valid = [sum(keep[b]) for b in range(B)]
    if slip == "masked_placeholder_counts":
        n_img = [sum(1 for t in range(T) if idl[b][t] == IMG) for b in range(B)]
    else:
        n_img = [sum(1 for t in range(T) if keep[b][t] and idl[b][t] == IMG) for b in range(B)]
    consumed = (lambda n: n) if slip == "no_index_for_imageless" else (lambda n: max(n, 1))
    # splice_len_kernel: thread `tid` owns sequences [tid * per, tid * per + per); an exclusive scan over the threads' sums, then a walk
    per = (B + CHUNK - 1) // CHUNK
    part, run = [], 0
    for tid in range(CHUNK):
        part.append(run)
        run += sum(consumed(n_img[b]) for b in range(tid * per, min(tid * per + per, B)))
    img_start, seq_len = [0] * B, [0] * B
    for tid in range(CHUNK):
        s = part[tid]
        for b in range(tid * per, min(tid * per + per, B)):
            n = n_img[b]
            img_start[b] = s
            rows = off[s + n] - off[s] if n > 0 and s + n <= n_images else 0
            ln = n_valid[b] - n + rows
            if max_length:
                ln = min(ln, max_length)
            seq_len[b] = ln
            if slip != "thread_prefix":
                s += consumed(n)
    max_len = max(seq_len)                                                  # the wrapper's one host read
    # splice_plan_kernel: one workgroup per sequence
    src = [[PAD] * max_len for _ in range(B)]
    new_lab = [[IGNORE] * max_len for _ in range(B)]
    new_mask = [[0] * max_len for _ in range(B)]
    new_pos = [[0] * max_len for _ in range(B)]
    for b in range(B):
        ln = seq_len[b]
        shift = max_len - ln if left else 0
        for q in range(ln):
            new_mask[b][shift + q] = 1
            new_pos[b][shift + q] = q
        run_img = run_w = 0
        for t0 in range(0, T, CHUNK):
            c_img = c_w = 0                                                 # the two scans of this chunk
            for t in range(t0, min(t0 + CHUNK, T)):
                if not keep[b][t]:
                    continue
                p0 = run_w + c_w
                if idl[b][t] == IMG:
                    im = img_start[b] + run_img + c_img
                    row0 = off[min(im, n_images)]
                    w = off[min(im + 1, n_images)] - row0
                    c_img += 1
                    if not (slip == "trunc_whole_image" and p0 + w > ln):
                        for r in range(w):
                            if p0 + r < ln:
                                src[b][shift + p0 + r] = -(row0 + r + 1)
                                new_lab[b][shift + p0 + r] = IGNORE
                else:
                    w = 1
                    if p0 < ln:
                        src[b][shift + p0] = idl[b][t]
                        if lab is not None:
                            l = lab[b][t]
                            new_lab[b][shift + p0] = IGNORE if (l == TARGET and slip != "target_kept") else l
                c_w += w
            if slip != "no_image_carry":
                run_img += c_img
            if slip != "no_chunk_carry":
                run_w += c_w

    def t2(x, dt):
        return torch.tensor(x, dtype=dt).reshape(B, max_len)
    return Plan(t2(src, torch.int32), None if labels is None else t2(new_lab, torch.int64), t2(new_mask, torch.int64), t2(new_pos, torch.int64),
                torch.tensor(seq_len, dtype=torch.int32), torch.tensor(img_start, dtype=torch.int32))


# ---- the oracle's plan and rows ----------------------------------------------------------------------------------------------------------------
COLS = {F32: slice(1, 5), BF16: slice(5, 13), F16: slice(13, 21)}
N_COLS = 21


@functools.lru_cache(maxsize=None)
def value_tables(n_image_rows, seed):
    """fp64 tables (V, 21) and (n_image_rows, 21).  Column 0 names the row: r for embedding row r, -(r + 1) for packed image row r.  Columns
    COLS[dt] hold seeded values of `dt`'s grid (every fp32 / bf16 / fp16 number is an fp64 number), so that the oracle's fp64 rows cast to `dt` are
    bit for bit the rows it gives on the tables cast to `dt`: it only copies rows and writes zeros.  One oracle call serves every dtype."""
    g = _gen(seed)
    W = torch.zeros(V, N_COLS, dtype=torch.float64)
    Fm = torch.zeros(n_image_rows, N_COLS, dtype=torch.float64)
    W[:, 0] = torch.arange(V, dtype=torch.float64)
    Fm[:, 0] = -(torch.arange(n_image_rows, dtype=torch.float64) + 1)
    for dt in DTS:
        W[:, COLS[dt]] = torch.randn(V, WIDTH[dt], generator=g).to(dt).double()
        Fm[:, COLS[dt]] = torch.randn(n_image_rows, WIDTH[dt], generator=g).to(dt).double()
    return W, Fm


def tables(image_lengths, dt, seed=7):
    """(embedding table (V, WIDTH[dt]), packed image tokens (rows, WIDTH[dt])) in `dt`: the columns of `value_tables` the oracle saw."""
    W, Fm = value_tables(sum(image_lengths), seed)
    return W[:, COLS[dt]].to(dt).contiguous(), Fm[:, COLS[dt]].to(dt).contiguous()


def split(packed, image_lengths):
    off = offsets(image_lengths)
    return [packed[off[i]:off[i + 1]] for i in range(len(image_lengths))]


def oracle_run(ids, mask, labels, image_lengths, max_length, left, pos_dtype=torch.int64, seed=7):
    """The oracle on the value tables.  Returns (position_ids, attention_mask, rows fp64 (B, max_len, 21), labels) as the oracle returns them,
    `mask` / `labels` None included; position ids are asked for in `pos_dtype`."""
    B, T = ids.shape
    W, Fm = value_tables(sum(image_lengths), seed)
    pos = torch.arange(T, dtype=pos_dtype).expand(B, T).clone()
    return O.splice_multimodal(ids, pos, mask, labels, split(Fm, image_lengths), W, max_length=max_length, padding_side="left" if left else "right")


def src_of(rows, new_mask):
    """`src` read back out of the oracle's rows: column 0 names the row, and a position the new mask leaves out is a zero row."""
    src = rows[..., 0].round().to(torch.int64)
    return torch.where(new_mask != 0, src, torch.full_like(src, PAD)).to(torch.int32)


def oracle_plan(ids, mask, labels, image_lengths, max_length, left):
    """Plan(src, labels, mask, position_ids, None, None) by the oracle, with an all-ones mask standing in for None (src needs the new mask)."""
    m = torch.ones_like(ids) if mask is None else mask
    pos, am, rows, lab = oracle_run(ids, m, labels, image_lengths, max_length, left)
    return Plan(src_of(rows, am), lab, am.to(torch.int64), pos, None, None), rows


def embeds_of(rows, dt):
    """The oracle's inputs_embeds for the tables of `dt`."""
    return rows[..., COLS[dt]].to(dt)


# ---- where the truncation lands ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def layout(name):
    """The untruncated right-padded plan of a program and, for its longest sequence b, the output positions [p0, p1) of that sequence's
    longest image, the last one among equals (None when no sequence has image rows)."""
    ids, am, labels, lengths, _ = program(name)
    plan = plan_emulate(ids, am, labels, lengths, None, False)
    b = int(plan.seq_len.argmax())
    row = plan.src[b].tolist()
    off = offsets(lengths)
    best = None
    for i in range(len(lengths)):
        ps = [p for p, s in enumerate(row) if s != PAD and s < 0 and off[i] <= -(s + 1) < off[i + 1]]
        if ps and (best is None or len(ps) >= best[1] - best[0]):
            best = (ps[0], ps[-1] + 1)
    return plan, b, best


def truncations(name):
    """name -> max_length, from the program's own layout.  `max_length = p + 1` makes position p the last one kept."""
    plan, b, span = layout(name)
    longest = int(plan.seq_len.max())
    out = {"one": 1, "above": longest + 5}
    if span is not None:
        p0, p1 = span
        text = [p for p, s in enumerate(plan.src[b].tolist()) if s >= 0 and p > 1]
        out.update(first_row=p0 + 1, middle_row=(p0 + p1) // 2 + 1, last_row=p1, after=p1 + 1, text=text[len(text) // 3] + 1)
    return {k: out[k] for k in TRUNCS if k in out}


RECORDED_PROGRAMS = [n for n in PROGRAMS if n != "nothing_kept"]
RECORDED = ["right", "trunc_left", "none"]


def recorded_case(name, case):
    """The calls whose outputs by the reference's own function are kept in tests/golden/splice_programs.npz (written by
    tests/golden/make_golden_splice_programs.py): (ids, mask, labels, image_lengths, max_length, left).  `right`: untruncated, right-padded;
    `trunc_left`: cut in the middle of an image, left-padded; `none`: `right` without position ids, mask and labels."""
    ids, am, labels, lengths, _ = unmasked(name) if case == "none" else program(name)
    if case == "trunc_left":
        return ids, am, labels, lengths, truncations(name)["middle_row"], True
    return ids, am, labels, lengths, None, False


def cases(names=PROGRAMS):
    """Every (program, truncation, side)."""
    return [(n, k, s) for n in names for k in truncations(n) for s in SIDES]
