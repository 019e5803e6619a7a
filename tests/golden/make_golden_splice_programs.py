"""Golden vectors of the splice programs (tests/golden/splice_programs.npz).

Run where the reference checkout is available:  python tests/golden/make_golden_splice_programs.py

The reference's own prepare_inputs_labels_for_multimodal (setokim_arch.py:213-355), run unmodified through oracle/rac_harness.py:
rac_prepare_inputs, on the programs of tests/splice_cases.py (every one but `nothing_kept`) with D = 4 fp32 tables: per program the untruncated
right-padded call, a call truncated inside an image and left-padded, and the first without position ids, mask and labels.  Stored: the specs and
the REFERENCE's outputs; the inputs regenerate from the programs' seeds.  Nothing of the reference's text is kept here: its module is loaded from
the checkout by the harness at run time."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(HERE))
import golden_io                 # noqa: E402
import rac_harness as R          # noqa: E402
import splice_cases as C         # noqa: E402


def npy(t):
    return t.detach().cpu().numpy()


def gen_splice_programs():
    arrs = {}
    for name in C.RECORDED_PROGRAMS:
        for case in C.RECORDED:
            ids, am, labels, lengths, max_length, left = C.recorded_case(name, case)
            B, T = ids.shape
            W, packed = C.tables(lengths, C.F32)
            pos = None if case == "none" else torch.arange(T).expand(B, T).clone()
            kw = dict(padding_side="left" if left else "right")
            if max_length is not None:
                kw["max_length"] = max_length
            rp, ra, re, rl = R.rac_prepare_inputs(ids, pos, am, labels, C.split(packed, lengths), W, **kw)
            key = f"{name}:{case}"
            arrs[key + ":spec"] = np.array([B, T, len(lengths), sum(lengths), -1 if max_length is None else max_length, 1 if left else 0])
            arrs[key + ":embeds"] = npy(re)
            if case == "none":
                assert rp is None and ra is None and rl is None
            else:
                arrs[key + ":pos"] = npy(rp); arrs[key + ":mask"] = npy(ra); arrs[key + ":labels"] = npy(rl)
            print(key, "reference output", tuple(re.shape))
    for path in golden_io.save(os.path.join(HERE, "splice_programs.npz"), **arrs):
        print(f"wrote {os.path.basename(path)}  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    gen_splice_programs()
