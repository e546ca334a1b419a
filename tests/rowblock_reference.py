"""The tests' reference for the row-block (MATMPIAIJ) set-up: the independent numpy / scipy statement of MatCreateScatters
(reference src/mc_sor.c:152-214; `rowblock_plan`) and of the level slicing of a hierarchy distributed by row blocks
(`rowblock_hierarchy`) that parmgmc_amd/csrc/pmg_rowblock.c is pinned to, index for index (tests/test_rowblock_c.py).  The
package itself builds every plan and every hierarchy in C; nothing here is imported by it."""


def rowblock_plan(ci_global, row0: int, row1: int, n_global: int, colors_owned, ncolors: int, extra_ghosts, rank: int, world: int, group=None):
    """Ghost set and per-colour ghost-update plan of one row block (what MatCreateScatters builds per colour in the
    reference, src/mc_sor.c:152-214; here de-duplicated per ghost row and laid out for ONE all-gather per colour).

    ci_global: the global column indices of this rank's rows; extra_ghosts: further global rows of other ranks whose
    values this rank reads (restriction / interpolation columns).  Returns (ghosts, plan) with ghosts = sorted global
    ids (local row nloc + q) and plan = dict(send_ptr, send_rows, counts, recv_ptr, recv_src, recv_rows): local OWNED rows
    this rank contributes per colour (by ascending global row), the ranks' block lengths, and for every ghost row the
    index of its value in the colour's gather buffer (blocks in rank order).  Collective over `group` (host objects)."""
    import numpy as np
    import torch.distributed as dist

    ci = np.asarray(ci_global, np.int64)
    nloc = row1 - row0
    off = ci[(ci < row0) | (ci >= row1)]
    extra = np.asarray(extra_ghosts, np.int64)
    extra = extra[(extra < row0) | (extra >= row1)]
    ghosts = np.unique(np.concatenate([off, extra]))
    ranges = [None] * world
    dist.all_gather_object(ranges, (row0, row1), group=group)
    starts = np.array([r[0] for r in ranges] + [n_global])
    assert all(ranges[r][1] == starts[r + 1] for r in range(world)), "row blocks must tile the rows in rank order"
    owner = np.searchsorted(starts, ghosts, side="right") - 1
    want = [ghosts[owner == p] for p in range(world)]  # global rows I need from rank p
    asked = [None] * world
    dist.all_gather_object(asked, want, group=group)  # asked[q][p] = rows rank q needs from rank p
    mycol = np.asarray(colors_owned, np.int64)
    assert len(mycol) == nloc and (nloc == 0 or (mycol.min() >= 0 and mycol.max() < ncolors))
    others = [np.asarray(asked[q][rank], np.int64) for q in range(world) if q != rank]
    needed = np.unique(np.concatenate(others)) if others else np.zeros(0, np.int64)  # my rows that another rank reads
    send_lists = [needed[mycol[needed - row0] == c] for c in range(ncolors)]  # sorted global rows, by colour
    all_lists = [None] * world
    dist.all_gather_object(all_lists, send_lists, group=group)
    counts = np.array([[len(all_lists[r][c]) for r in range(world)] for c in range(ncolors)], np.int64).reshape(ncolors, world)
    offs = np.concatenate([np.zeros((ncolors, 1), np.int64), np.cumsum(counts, axis=1)[:, :-1]], axis=1)
    send_ptr = np.concatenate([[0], np.cumsum([len(l) for l in send_lists])]).astype(np.int64)
    send_rows = (np.concatenate(send_lists) - row0 if send_ptr[-1] else np.zeros(0)).astype(np.int32)
    rsrc, rrow, rptr = [], [], [0]
    for c in range(ncolors):
        for p in range(world):
            if p == rank or not len(want[p]):
                continue
            lst = np.asarray(all_lists[p][c], np.int64)
            if not len(lst):
                continue
            k = np.searchsorted(lst, want[p])
            hit = (k < len(lst)) & (lst[np.minimum(k, len(lst) - 1)] == want[p])  # my ghosts owned by p that have colour c
            rsrc.append(offs[c, p] + k[hit])
            rrow.append(nloc + np.searchsorted(ghosts, want[p][hit]))
        rptr.append(sum(len(a) for a in rsrc))
    plan = dict(send_ptr=send_ptr, send_rows=send_rows, counts=np.ascontiguousarray(counts),
                recv_ptr=np.asarray(rptr, np.int64),
                recv_src=(np.concatenate(rsrc) if rsrc else np.zeros(0)).astype(np.int32),
                recv_rows=(np.concatenate(rrow) if rrow else np.zeros(0)).astype(np.int32))
    assert plan["recv_ptr"][-1] == len(ghosts), "every ghost row is owned by exactly one rank and has exactly one colour"
    return ghosts, plan


def rowblock_hierarchy(operators, interpolations, colorings, rank: int, world: int, starts=None, replicate_below: int = 50000, group=None):
    """This rank's share of a hierarchy distributed by row blocks -- host arrays only, no device, no C call; collective
    (the ghost plans of rowblock_plan).  operators / interpolations as for MGMC.from_hierarchy (level 0 = coarsest),
    colorings[l] = (colours of ALL rows of level l, number of colours) for the levels that will be row blocks (None below).
    Returns dict(fold, starts, n, levels): levels[l] for l >= fold holds the local operator (rp, ci, v: owned rows in
    global order, entries in global CSR order, then one identity row per ghost), colors (owned rows), ncolors, plan,
    ghosts (sorted global rows), nowned, row0, P (owned rows of P_l, columns in the local numbering of level l-1 -- global
    when that level is replicated) and R (the rows of P_l^T this rank owns on level l-1, columns in the local numbering of
    level l, entries by ascending global fine row).  Levels below `fold` are replicated (levels[l] = None)."""
    import numpy as np
    import scipy.sparse as sp

    L = len(operators)
    assert L >= 2 and len(interpolations) == L
    A = [sp.csr_matrix((np.asarray(v, np.float64), np.asarray(ci, np.int64), np.asarray(rp, np.int64)), shape=(len(rp) - 1, len(rp) - 1)) for rp, ci, v in operators]
    P = [None] + [sp.csr_matrix((np.asarray(interpolations[l][2], np.float64), np.asarray(interpolations[l][1], np.int64), np.asarray(interpolations[l][0], np.int64)), shape=(A[l].shape[0], A[l - 1].shape[0])) for l in range(1, L)]
    n = [a.shape[0] for a in A]
    if starts is None:
        starts = [np.linspace(0, n[l], world + 1).astype(np.int64) for l in range(L)]
    starts = [np.asarray(s_, np.int64) for s_ in starts]
    r0 = [int(s_[rank]) for s_ in starts]
    r1 = [int(s_[rank + 1]) for s_ in starts]
    R = [None] + [P[l].T.tocsr() for l in range(1, L)]  # rows of P^T, entries by ascending fine row
    for m in R[1:]:
        m.sort_indices()
    fold = 1  # lowest row-block level; the levels below are replicated
    while fold < L - 1 and n[fold] <= replicate_below:
        fold += 1
    ghosts, nloc = [np.zeros(0, np.int64)] * L, [r1[l] - r0[l] for l in range(L)]
    local_of = [None] * L  # global row -> local row of this rank (owned, then ghosts), -1 elsewhere; replicated levels: identity
    for l in range(fold):
        local_of[l] = np.arange(n[l], dtype=np.int64)
    levels = [None] * L
    for l in range(fold, L):
        col, ncol = colorings[l]
        col = np.asarray(col)
        mine = A[l][r0[l]:r1[l]]
        extra = [R[l][r0[l - 1]:r1[l - 1]].indices.astype(np.int64)]  # fine rows my restriction rows read (level l-1 replicated: the block I restrict into)
        if l + 1 < L:
            extra.append(P[l + 1][r0[l + 1]:r1[l + 1]].indices.astype(np.int64))  # rows of this level the finer level's interpolation reads
        ghosts[l], plan = rowblock_plan(mine.indices, r0[l], r1[l], n[l], col[r0[l]:r1[l]], ncol, np.concatenate(extra), rank, world, group)
        ng = len(ghosts[l])
        lo = np.full(n[l], -1, np.int64)
        lo[r0[l]:r1[l]] = np.arange(nloc[l])
        lo[ghosts[l]] = nloc[l] + np.arange(ng)
        local_of[l] = lo
        # local operator: my rows (entries in the order of the global CSR row) + one identity row per ghost
        rp = np.concatenate([mine.indptr, mine.indptr[-1] + 1 + np.arange(ng)]).astype(np.int32)
        ci = np.concatenate([lo[mine.indices], nloc[l] + np.arange(ng)]).astype(np.int32)
        assert ci.min(initial=0) >= 0
        v = np.concatenate([mine.data, np.ones(ng)])
        levels[l] = dict(rp=rp, ci=ci, v=v, colors=np.ascontiguousarray(col[r0[l]:r1[l]], np.int32), ncolors=int(ncol), plan=plan, ghosts=ghosts[l], nowned=nloc[l], row0=r0[l])
    for l in range(fold, L):
        pm = P[l][r0[l]:r1[l]]  # my rows of P_l (entries in the caller's order), columns -> local numbering of level l-1
        prp, pci, pv = pm.indptr.astype(np.int32), local_of[l - 1][pm.indices].astype(np.int32), np.ascontiguousarray(pm.data)
        rm = R[l][r0[l - 1]:r1[l - 1]]  # the rows of P_l^T I own on level l-1, columns -> local numbering of level l
        rrp, rci, rv = rm.indptr.astype(np.int32), local_of[l][rm.indices].astype(np.int32), np.ascontiguousarray(rm.data)
        assert pci.min(initial=0) >= 0 and rci.min(initial=0) >= 0, "a transfer reads a row that is neither owned nor a ghost"
        levels[l]["P"] = (prp, pci, pv)
        levels[l]["R"] = (rrp, rci, rv)
        levels[l]["ncoarse_local"] = n[l - 1] if l == fold else nloc[l - 1] + len(ghosts[l - 1])
    return dict(fold=fold, starts=starts, n=n, levels=levels)
