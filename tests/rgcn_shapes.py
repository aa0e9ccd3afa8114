"""The shapes the typed SpMM kernel pair (csrc/dcr_spmm.hip) is run at, and the dispatch that turns a shape into a kernel
instantiation, restated: plain Python, no torch, no GPU, so that tests/test_rgcn_cpu.py can say which of the 15 (LPR, VEC)
instantiations tests/test_rgcn_gpu.py launches."""

VECS = (4, 2, 1)
LPRS = (4, 8, 16, 32, 64)                     # pick_lpr_vec: the first LPR that holds a row's VEC-wide pieces, else 64
# The first nine: every VEC path, 260 > one group's stride of 64 lanes x 4.  Then one width per instantiation those never reach
# (VEC 4 on 8 lanes; VEC 1 and VEC 2 on 8 to 64), and 130 / 65: a second trip of the f0 loop at VEC 2 / VEC 1 (64 lanes x VEC).
N_FEATS = [1, 2, 3, 4, 6, 7, 64, 68, 260, 20, 13, 17, 10, 18, 34, 66, 130, 65]
# floats added to both leading dimensions.  1: odd, VEC 1 at every width; 2: = 2 (mod 4), VEC 2 where the width allows VEC 4
PADS = (0, 1, 2)
FULL_ROWS = 70                                # holds the whole row pattern and more than one workgroup at every LPR


def vec_lpr(n_feat, *lds, residues=()):
    """(VEC, LPR) of the dispatch of both entry points: the widest VEC that divides the width, every leading dimension and
    every operand pointer the entry point looks at (``residues``: their byte addresses modulo 16; none: all aligned)."""
    vec = next(v for v in VECS if n_feat % v == 0 and all(ld % v == 0 for ld in lds) and all(r % (4 * v) == 0 for r in residues))
    return vec, next((lpr for lpr in LPRS[:-1] if n_feat // vec <= lpr), LPRS[-1])


def groups(n_feat, *lds, residues=()):
    """Rows per workgroup = lane groups summing a hub row."""
    return 256 // vec_lpr(n_feat, *lds, residues=residues)[1]


def row_counts(n_feat, *lds):
    g = groups(n_feat, *lds)
    return [g - 1, g, g + 1, FULL_ROWS]


def leading_dims(n_feat, n_rel, self_block, pad):
    """(wide, narrow): the leading dimensions of the operand with (n_rel + self_block) column blocks and of the one-block one."""
    return (n_rel + self_block) * n_feat + pad, n_feat + pad


def path(n_feat, wide, narrow):
    """What of the kernels a shape exercises: (VEC, LPR, the f0 loop takes more than one trip, a leading dimension and not the
    width narrowed VEC)."""
    vec, lpr = vec_lpr(n_feat, wide, narrow)
    return vec, lpr, n_feat > vec * lpr, vec != vec_lpr(n_feat)[0]


def paths(n_feats=N_FEATS, pads=PADS):
    return {path(f, *leading_dims(f, n_rel, self_block, pad)) for f in n_feats for pad in pads for n_rel in (1, 2, 3, 8)
            for self_block in (0, 1)}
