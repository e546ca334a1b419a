"""Multi-GPU drivers: one process per GPU, torch.distributed for the bootstrap (and for the fall-back transport).

Replaces the reference's MPI design -- row-block ownership of a MATMPIAIJ with one ghost VecScatter per colour
(reference src/mc_sor.c:317-340, scatter plan :152-214):

* ``DistGridSampler`` -- sorgibbs / mcgibbs on the DMDA operator, z-slabs (`slab_cuts`, PETSc's ownership rule).  The
  sample loop is the C loop of pmg_dist.c over the "ipc" transport (peer stores + flag words, hand-shake inside the
  sweep kernel) or RCCL send/recv (``SlabDriver``); ``run_samples`` + ``SlabHalo`` is the same
  schedule over torch.distributed point-to-point ops (RCCL tensors, or gloo through host memory in the CPU tests).
* ``DistMGMC`` -- the Multigrid Monte Carlo V-cycle on z-slabs (pmg_mgmc_create_dmda_slab), incl. low-rank updates.
* ``DistMCSOR`` -- general MATAIJ matrices by row blocks: per-colour device sweeps, ghost updates between them.
* ``DistAIJMGMC`` / ``CRowBlock`` -- MGMC on a hierarchy of MATAIJ levels by row blocks (``_RowBlockMGMC``).

One bootstrap: every class gets its "ipc" or "rccl" transport from ``SlabDriver``, that is from pmg_dist_create_comm of
pmg_rowblock.c over a byte all-gather on torch.distributed -- the call the adapter makes over MPI_Allgather; the
agreements after each step that can fail on one rank alone, and the tear-down of a half-built transport, are the
library's.  Python adds two things.  ``_agree_on_driver`` falls back from one transport to the next (ipc -> rccl ->
torch P2P) after the driver's ``selftest()``, a local round trip that can fail on one rank alone.  ``_teardown`` is the one
tear-down order (disconnect, device synchronise, barrier, free); it is Python, not pmg_dist_destroy_comm, because after a
failed agreement a rank WITHOUT an object must join it, and such a rank can only be met through torch.distributed.

Because noise is a function of global indices only, every chain is the single-device chain for any number of ranks.
torch is plumbing here: the sweeps are the HIP kernels behind the C-ABI.
"""
from __future__ import annotations

from .capi import SOR_FORWARD_SWEEP, directions
from .slab import slab_cuts


class SlabHalo:
    """Ghost-plane exchange of one colour of a flat colour-partitioned vector with the z-neighbours.

    `planes[color][side] = (owned_offset, ghost_offset, count)` as returned by ``pmg_grid_halo_plane``."""

    def __init__(self, rank: int, world: int, planes, group=None):
        self.rank, self.world, self.planes, self.group = rank, world, planes, group

    def start(self, y, color: int):
        import torch
        import torch.distributed as dist

        # RCCL ("nccl") moves device memory directly over xGMI.  The gloo backend (CPU tests, and the two-ranks-
        # on-one-GPU test where RCCL cannot be used) needs host buffers: stage device planes through the host.
        staged = y.is_cuda and dist.get_backend(self.group) == "gloo"
        ops, post = [], []
        for side, peer in ((0, self.rank - 1), (1, self.rank + 1)):
            if peer < 0 or peer >= self.world:
                continue
            own, ghost, n = self.planes[color][side]
            if staged:
                snd, rcv = y[own:own + n].cpu(), torch.empty(n, dtype=y.dtype)
                post.append((ghost, n, rcv))
            else:
                snd, rcv = y[own:own + n], y[ghost:ghost + n]
            ops.append(dist.P2POp(dist.isend, snd, peer, self.group))
            ops.append(dist.P2POp(dist.irecv, rcv, peer, self.group))
        reqs = dist.batch_isend_irecv(ops) if ops else []
        return (reqs, post, y) if staged else reqs

    @staticmethod
    def finish(reqs):
        if isinstance(reqs, tuple):
            works, post, y = reqs
            for r in works:
                r.wait()
            for ghost, n, rcv in post:
                y[ghost:ghost + n].copy_(rcv)
            return
        for r in reqs:
            r.wait()

    def exchange(self, y, color: int):
        self.finish(self.start(y, color))


def color_schedule(sweep_type: int):
    """Colour order of every directional sweep of one sample (capi.directions): forward = colours 0,1; backward = 1,0
    (reference src/mc_sor.c:257,274)."""
    return [(0, 1) if d == SOR_FORWARD_SWEEP else (1, 0) for d in directions(sweep_type)]


def run_samples(sweep_planes, halo: SlabHalo, nz: int, b, y, its: int, sweep_type: int, counter0: int) -> int:
    """The distributed sample loop with communication/computation overlap.

    sweep_planes(color, kbegin, kcount, b, y, counter) sweeps the local points of one colour on owned planes
    [kbegin, kbegin+kcount) (HIP kernel in production, an injected CPU kernel in the gloo tests).

    Invariant: the ghost planes of colour c are current once the exchange started after the last sweep of colour
    c has completed.  Per colour c: wait for the exchange of colour 1-c; sweep the two boundary planes (the only
    ones that read ghost planes); start the exchange of colour c; sweep the interior planes while it is in
    flight -- the overlap PCPARSOR gets by starting `botsct` before its INT1 rows (reference
    src/pc_parsor.c:739-745), here per colour instead of the reference's blocking per-colour VecScatter
    (src/mc_sor.c:318-319)."""
    pending = {0: halo.start(y, 0), 1: halo.start(y, 1)}  # the caller's y has no ghost values yet
    edge = sorted({0, nz - 1})
    ctr = counter0
    for _ in range(its):
        for order in color_schedule(sweep_type):
            for c in order:
                halo.finish(pending[1 - c])  # colour c reads colour 1-c across the slab faces
                pending[1 - c] = []
                for k in edge:
                    sweep_planes(c, k, 1, b, y, ctr)
                halo.finish(pending[c])  # an older exchange of colour c must not land after the new one starts
                pending[c] = halo.start(y, c)
                if nz > 2:
                    sweep_planes(c, 1, nz - 2, b, y, ctr)
            ctr += 1
    halo.finish(pending[0])
    halo.finish(pending[1])
    return ctr


def _all_ok(err, group, what: str) -> None:
    """Agreement point: raises on EVERY rank if `err` is set on any rank (all-reduce MIN of an ok flag)."""
    import torch
    import torch.distributed as dist

    flag = torch.tensor([0 if err else 1], device="cuda" if dist.get_backend(group) == "nccl" else "cpu")
    dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
    if int(flag.item()) != 1:
        raise RuntimeError(f"{what}: {err or 'failed on another rank'}")


def _teardown(drv, world: int, group) -> None:
    """Orderly end of a transport, COLLECTIVE over all ranks of `group` -- entered by every rank whether or not it holds
    a driver (drv None: its constructor failed on this rank alone): unmap the peers' blocks, barrier, free the own block.
    A rank that frees a block a peer still has mapped and exports a fresh one at once gets "invalid argument" from
    hipIpcGetMemHandle; a rank that skipped the barrier would meet its peers in a different collective.  This stays Python
    (pmg_dist_destroy_comm is the adapter's): falling back from one transport to the next needs a tear-down that a rank
    without an object can join, and such a rank has only torch.distributed to join it through."""
    if drv is not None and getattr(drv, "_h", None):
        drv.disconnect()
    if world > 1:
        import torch
        import torch.distributed as dist

        if torch.cuda.is_available():
            torch.cuda.synchronize()
        dist.barrier(group=group)
    if drv is not None:
        drv.free()


def _agree_on_driver(candidates, make, rank: int, world: int, group, what: str):
    """Try the transports in order; every rank must end up on the same one.  make(name) builds a driver (collective
    internally: it raises on every rank together), then the driver's `selftest()`, if it has one, runs -- LOCAL, so it may
    fail on one rank alone; its exception is kept, not propagated, and the object held.  Success is agreed with an
    all-reduce, and after a failed agreement EVERY rank -- with or without a driver of its own -- runs the same collective
    tear-down before the next candidate's constructor starts its own collectives.  Returns (driver, name) or (None, None)."""
    import torch
    import torch.distributed as dist

    dev = "cuda" if dist.get_backend(group) == "nccl" else "cpu"
    for cand in candidates:
        drv, err = None, None
        try:
            drv = make(cand)
            if hasattr(drv, "selftest"):
                drv.selftest()
        except Exception as e:  # noqa: BLE001
            err = e
        flag = torch.tensor([0 if err else 1], device=dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
        if int(flag.item()) == 1:
            return drv, cand
        _teardown(drv, world, group)
        if rank == 0:
            print(f"[parmgmc_amd] {what}: transport '{cand}' unavailable ({err if err else 'on another rank'}); trying the next one", flush=True)
    return None, None


class SlabDriver:
    """A transport object of pmg_dist.c and its C sample loop, no Python in the loop.  kind "ipc": boundary planes are
    stored device-to-device straight into the neighbour's receive block (hipIpc memory) and announced by flag words;
    kind "rccl": RCCL send/recv called straight from the host library, comm stream + events.  Both are built by
    the library's collective bootstrap (pmg_rowblock.c) over a byte all-gather on torch.distributed: it agrees after every
    step that can fail on one rank alone and raises PMGError ("... failed on rank r") on EVERY rank together, the half-built objects torn
    down in step.  grid None: a transport without a slab.  loopback (world 1): the rank is its own z-neighbour for the
    halo, nothing is collective."""

    def __init__(self, kind: str, grid, rank: int, world: int, group=None, loopback: bool = False):
        import ctypes as C

        from . import capi
        from .capi import check, lib

        self._h = C.c_void_p()
        self.kind, self._grid, self._rank = kind, grid, rank  # the grid is kept alive
        self._world, self._group = (1 if loopback else world), group
        g = grid._h if grid is not None else None
        path = capi.torch_rccl_path()
        path = path.encode() if path else None
        if loopback and kind == "ipc":
            check(lib.pmg_dist_create_ipc(g, 0, 1, C.byref(self._h)))
            check(lib.pmg_dist_ipc_connect_loopback(self._h))
        elif loopback:
            uid = C.create_string_buffer(128)
            check(lib.pmg_dist_get_unique_id(path, uid))
            check(lib.pmg_dist_create(g, rank, world, uid, path, 1, C.byref(self._h)))
        else:
            self._comm = capi.torch_host_comm(rank, world, group)  # (pmg_host_comm, its callback): alive as long as the handle
            check(lib.pmg_dist_create_comm(C.byref(self._comm[0]), kind.encode(), g, path, C.byref(self._h)))

    def selftest(self):
        """ipc only (ncclCommInitRank has connected RCCL's peers itself).  One round trip of a known pattern with both
        z-neighbours (peer copies into their blocks, flag words, copy out) plus the all-gather pattern: if peer access or
        the flags do not work on this machine this raises -- on every rank, the wait gives up after about a minute -- and
        _agree_on_driver moves on to the next transport.  LOCAL: it can fail on one rank alone and no collective follows."""
        if self.kind != "ipc":
            return
        import ctypes as C

        import torch

        from .capi import check, lib
        from .wrappers import _ptr, _stream

        rank, world = self._rank, self._world
        n = 4096
        send = torch.full((2, n), float(rank + 1), dtype=torch.float64, device="cuda") + torch.arange(n, dtype=torch.float64, device="cuda") / n
        recv = torch.zeros((2, n), dtype=torch.float64, device="cuda")
        P, I64 = C.c_void_p * 1, C.c_int64 * 1
        nn = I64(n)
        check(lib.pmg_dist_exchange(self._h, 1, P(_ptr(send[0])), nn, P(_ptr(recv[0])), nn, P(_ptr(send[1])), nn, P(_ptr(recv[1])), nn, _stream()))
        torch.cuda.synchronize()
        frac = torch.arange(n, dtype=torch.float64, device="cuda") / n
        if rank > 0 and not torch.equal(recv[0], float(rank) + frac):
            raise RuntimeError("ipc halo self-test: wrong data from the low neighbour")
        if rank < world - 1 and not torch.equal(recv[1], float(rank + 2) + frac):
            raise RuntimeError("ipc halo self-test: wrong data from the high neighbour")
        # all-gather (all-peer mappings for more than two ranks): rank r contributes 64 + r values
        counts = [64 + r for r in range(world)]
        offs = [sum(counts[:r]) for r in range(world)]
        buf = torch.zeros(sum(counts), dtype=torch.float64, device="cuda")
        buf[offs[rank]:offs[rank] + counts[rank]] = float(rank + 1)
        A64 = C.c_int64 * world
        check(lib.pmg_dist_allgather(self._h, _ptr(buf), A64(*offs), A64(*counts), _stream()))
        torch.cuda.synchronize()
        want = torch.cat([torch.full((counts[r],), float(r + 1), dtype=torch.float64, device="cuda") for r in range(world)])
        if not torch.equal(buf, want):
            raise RuntimeError("ipc halo self-test: all-gather returned wrong data")

    def sample_cvec(self, b, y, its, scaled, sweep_type, seed, counter0):
        import ctypes as C

        from .capi import check, lib
        from .wrappers import _ptr, _stream

        out = C.c_uint64()
        check(lib.pmg_dist_sample_cvec(self._h, _ptr(b), _ptr(y), its, int(scaled), sweep_type, seed, counter0, C.byref(out), _stream()))
        return out.value

    def check(self):
        """after torch.cuda.synchronize(): raises if a device-side wait for a halo flag gave up"""
        from .capi import check, lib

        check(lib.pmg_dist_check(self._h))

    def describe(self, lo_device: int = -1, hi_device: int = -1) -> dict:
        """pmg_dist_describe: device, PCI bus id, peer access to the z-neighbours' devices, transport, ncclCommCount, halo
        wait polls -- this rank's entry of the multi-GPU bench record"""
        import ctypes as C

        from .capi import DistDescription, check, lib

        d = DistDescription()
        check(lib.pmg_dist_describe(self._h, lo_device, hi_device, C.byref(d)))
        return d.as_dict()

    def disconnect(self):
        """local: unmap the peers' receive blocks"""
        from .capi import lib

        if self._h:
            lib.pmg_dist_ipc_disconnect(self._h)

    def free(self):
        """local: free the handle and the own receive block (after every peer has unmapped it)"""
        import ctypes as C

        from .capi import lib

        if self._h:
            lib.pmg_dist_destroy(C.byref(self._h))

    def destroy(self):
        """Collective, orderly tear-down: unmap the peers' blocks, barrier, free the own block."""
        if self._h:
            _teardown(self, self._world, self._group)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def RcclSlabDriver(grid, rank: int, world: int, loopback: bool = False, group=None):
    return SlabDriver("rccl", grid, rank, world, group, loopback)


def IpcSlabDriver(grid, rank: int, world: int, group=None, loopback: bool = False):
    return SlabDriver("ipc", grid, rank, world, group, loopback)


class DistGridSampler:
    """sorgibbs/mcgibbs sampler for the grid operator on `world` GPUs (this process = one slab).

    transport "rccl" (default when torch.distributed runs on the nccl backend): the C loop of pmg_dist.c;
    transport "torch": the Python loop `run_samples` over torch.distributed P2P (gloo in the CPU tests; also the
    automatic fall-back if RCCL cannot be initialised)."""

    def __init__(self, nx, ny, nz, kappa, rank, world, omega=1.0, sweep_type=SOR_FORWARD_SWEEP, scaled=True, group=None, transport=None):
        import os

        from .wrappers import GridMCSOR

        cuts = slab_cuts(nz, world)
        self.rank, self.world = rank, world
        self.grid = GridMCSOR(nx, ny, nz, kappa, kz0=cuts[rank], nz_owned=cuts[rank + 1] - cuts[rank])
        self.grid.set_omega(omega)
        self.sweep_type, self.scaled = sweep_type, scaled
        planes = [[self.grid.halo_plane(c, s) for s in (0, 1)] for c in (0, 1)]
        self.halo = SlabHalo(rank, world, planes, group)
        self.rccl = None
        self.transport = "none" if world == 1 else "torch"
        want = transport or os.environ.get("PMG_DIST_TRANSPORT")
        if world > 1 and want != "torch":
            import torch
            import torch.distributed as dist

            on_gpu = dist.get_backend(group) == "nccl"
            # preference: ipc (peer copies, lowest latency) -> rccl (ncclSend/ncclRecv) -> torch P2P; every rank must
            # take the same path, so success is agreed with an all-reduce after each attempt
            candidates = [want] if want else (["ipc", "rccl"] if on_gpu else [])
            drv, name = _agree_on_driver(candidates, lambda cand: SlabDriver(cand, self.grid, rank, world, group), rank, world, group, "halo exchange")
            if drv is not None:
                self.rccl, self.transport = drv, name

    def check(self):
        """after torch.cuda.synchronize(): raises if the halo transport lost a neighbour"""
        if self.rccl is not None:
            self.rccl.check()

    def describe(self, lo_device: int = -1, hi_device: int = -1) -> dict:
        """this rank's entry of a multi-GPU bench record (see SlabDriver.describe); the torch P2P loop has no C object"""
        if self.rccl is not None:
            return self.rccl.describe(lo_device, hi_device)
        import torch

        dev = torch.cuda.current_device() if torch.cuda.is_available() else -1
        pci = "unknown"
        try:
            p = torch.cuda.get_device_properties(dev)
            pci = f"{p.pci_domain_id:04x}:{p.pci_bus_id:02x}:{p.pci_device_id:02x}.0"
        except Exception:  # noqa: BLE001
            pass
        return {"rank": self.rank, "nranks": self.world, "device": dev, "pci_bus_id": pci, "neighbour_ranks": [self.rank - 1 if self.rank > 0 else -1, self.rank + 1 if self.rank < self.world - 1 else -1], "peer_access_lo_hi": [-1, -1], "transport": self.transport, "rccl_comm_count": 0, "halo_wait_polls": 0}

    def destroy(self):
        """collective: orderly tear-down of the halo transport (call on every rank before building another one)"""
        if self.rccl is not None:
            self.rccl.destroy()
            self.rccl = None

    def sample_cvec(self, b, y, its: int, seed: int, counter0: int = 0) -> int:
        if self.world == 1:
            self.grid.set_sweep_type(self.sweep_type)
            return self.grid.sample_cvec(b, y, its, seed, counter0, self.scaled)
        if self.rccl:
            return self.rccl.sample_cvec(b, y, its, self.scaled, self.sweep_type, seed, counter0)
        g = self.grid
        return run_samples(lambda c, k0, nk, bb, yy, ctr: g.sweep_color_planes_cvec(c, k0, nk, bb, yy, True, self.scaled, seed, ctr), self.halo, g.nz, b, y, its, self.sweep_type, counter0)


class DistMGMC:
    """Multigrid Monte Carlo on `world` GPUs (this process = one z-slab of every distributed level): the C V-cycle of
    pmg_mgmc.c on top of the halo transport of pmg_dist.c ("ipc" or "rccl"; reference PCGAMGMC over MPI ranks,
    src/pc_gamgmc.c + src/mc_sor.c:298-381).  b and y of `sample` are this rank's planes in natural order."""

    def __init__(self, nx, ny, nz, kappa, levels, rank, world, group=None, transport=None):
        import ctypes as C

        import numpy as np

        from .capi import check, lib
        from .wrappers import MGMC

        self.rank, self.world = rank, world
        self.cuts = slab_cuts(nz, world)
        if world == 1:
            self.grid_sampler, self.transport = None, "none"
            self.mg = MGMC(nx, ny, nz, kappa, levels)
        else:
            self.grid_sampler = DistGridSampler(nx, ny, nz, kappa, rank, world, group=group, transport=transport)
            self.transport = self.grid_sampler.transport
            if self.grid_sampler.rccl is None:
                raise RuntimeError("the distributed V-cycle needs the ipc or rccl halo transport (torch P2P carries only the stand-alone sweeps)")
            cuts = np.asarray(self.cuts, np.int32)
            mg = MGMC.__new__(MGMC)
            mg.nx, mg.ny, mg.nz, mg.levels = nx, ny, nz, levels
            mg._h = C.c_void_p()
            check(lib.pmg_mgmc_create_dmda_slab(nx, ny, nz, kappa, levels, self.grid_sampler.grid._h, self.grid_sampler.rccl._h, cuts.ctypes.data, C.byref(mg._h)))
            mg.n = nx * ny * (self.cuts[rank + 1] - self.cuts[rank])
            self.mg = mg
        self.n_local = nx * ny * (self.cuts[rank + 1] - self.cuts[rank])
        self.plane_range = (self.cuts[rank], self.cuts[rank + 1])

    def __getattr__(self, name):  # set_smoother, set_coarse, set_correction_form, setup, sample, ...
        return getattr(self.mg, name)

    def destroy(self):
        self.mg.destroy()  # before the transport and the grid it borrows
        if self.grid_sampler is not None:
            self.grid_sampler.destroy()
        self.grid_sampler = None


def _c_rowblock_plan(rank: int, world: int, group, starts, ci, colors, ncolors: int):
    """pmg_rowblock_plan_create for this rank's rows (ci: their global columns, int64; no transfer ghosts), read back with
    pmg_rowblock_plan_get: (ghosts, dict(send_ptr, send_rows, counts[ncolors, world], recv_ptr, recv_src, recv_rows)) as
    numpy copies.  Collective over `group`."""
    import ctypes as C

    import numpy as np

    from . import capi
    from .capi import check, lib

    comm, _keep = capi.torch_host_comm(rank, world, group)
    col = np.ascontiguousarray(colors, np.int32)
    pl, ng, ptrs = C.c_void_p(), C.c_int32(), [C.c_void_p() for _ in range(7)]
    check(lib.pmg_rowblock_plan_create(C.byref(comm), starts.ctypes.data, len(ci), ci.ctypes.data, 0, None, ncolors, col.ctypes.data, C.byref(pl)))
    try:
        check(lib.pmg_rowblock_plan_get(pl, C.byref(ng), *[C.byref(p_) for p_ in ptrs]))

        def arr(k, n, ct):
            return np.ctypeslib.as_array(C.cast(ptrs[k], C.POINTER(ct)), shape=(n,)).copy() if n else np.zeros(0, ct)

        send_ptr = arr(1, ncolors + 1, C.c_int64)
        plan = dict(send_ptr=send_ptr, send_rows=arr(2, int(send_ptr[-1]), C.c_int32), counts=arr(3, ncolors * world, C.c_int64).reshape(ncolors, world),
                    recv_ptr=arr(4, ncolors + 1, C.c_int64), recv_src=arr(5, ng.value, C.c_int32), recv_rows=arr(6, ng.value, C.c_int32))
        return arr(0, ng.value, C.c_int64), plan
    finally:
        lib.pmg_rowblock_plan_destroy(C.byref(pl))


def _rbh_mgmc(comm, transport, levels, replicate_below: int, coloring: int = 0):
    """The pmg_rbh_* call sequence of a hierarchy of MATMPIAIJ levels: levels[l] = dict(n=global rows, row0=, A=(rowptr,
    colidx_global, vals) of this rank's rows, P=(rowptr, colidx_global_coarse, vals) of this rank's rows of P_l (l >= 1)),
    level 0 = coarsest; the C side copies them.  Returns (rbh, mgmc): the pmg_mgmc handle borrows the hierarchy's arrays
    until its set-up, destroy rbh after it.  Collective over the ranks of `comm`."""
    import ctypes as C

    import numpy as np

    from .capi import check, lib

    rbh, mg = C.c_void_p(), C.c_void_p()
    check(lib.pmg_rbh_create(C.byref(comm), len(levels), replicate_below, C.byref(rbh)))
    try:
        if coloring:  # 0: the library's default rule
            check(lib.pmg_rbh_set_coloring(rbh, int(coloring)))
        for l, Lv in enumerate(levels):
            rp, ci, v = (np.ascontiguousarray(a_, t_) for a_, t_ in zip(Lv["A"], (np.int64, np.int64, np.float64)))
            check(lib.pmg_rbh_set_level_operator(rbh, l, Lv["n"], Lv["row0"], len(rp) - 1, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, 64))
            if l >= 1:
                prp, pci, pv = (np.ascontiguousarray(a_, t_) for a_, t_ in zip(Lv["P"], (np.int64, np.int64, np.float64)))
                check(lib.pmg_rbh_set_level_interpolation(rbh, l, len(prp) - 1, prp.ctypes.data, pci.ctypes.data, pv.ctypes.data, 64))
        check(lib.pmg_rbh_build(rbh))
        check(lib.pmg_rbh_create_mgmc(rbh, transport, C.byref(mg)))
    except Exception:
        lib.pmg_rbh_destroy(C.byref(rbh))
        raise
    return rbh, mg


class _RowBlockMGMC:
    """The pmg_mgmc object of a row-block hierarchy (`levels` as for _rbh_mgmc) on the transport `drv`, a SlabDriver that
    its owner keeps and destroys AFTER this object.  Collective over the driver's group, from creation to set-up."""

    def __init__(self, drv, levels, replicate_below: int, coloring: int = 0):
        import ctypes as C

        import numpy as np

        from .capi import RbhLevelView, check, lib

        self._group, self._h = drv._group, None
        self._rbh, self._h = _rbh_mgmc(drv._comm[0], drv._h, levels, replicate_below, coloring)
        fold, views = C.c_int32(), [RbhLevelView() for _ in levels]
        check(lib.pmg_rbh_get_info(self._rbh, None, C.byref(fold)))
        for l, v_ in enumerate(views):
            check(lib.pmg_rbh_get_level(self._rbh, l, C.byref(v_)))
        self.fold, self.starts = fold.value, [np.ctypeslib.as_array(v_.starts, shape=(drv._world + 1,)).copy() for v_ in views]
        top = views[-1]
        self.n_owned, self.n_local = top.nowned, top.nlocal
        self.row_range = (top.row0, top.row0 + top.nowned)
        self.levels = len(levels)

    def set_smoother(self, scaled: bool, omega: float = 1.0, sweep_type: int = SOR_FORWARD_SWEEP, its: int = 1):
        from .capi import check, lib

        check(lib.pmg_mgmc_set_smoother(self._h, int(scaled), omega, sweep_type, its))

    def set_correction_form(self, literal: bool):
        from .capi import check, lib

        check(lib.pmg_mgmc_set_correction_form(self._h, int(literal)))

    def algorithmic_bytes(self):
        """(this rank's algorithmic bytes of one sample, per level): pmg_mgmc_get_algorithmic_bytes"""
        import ctypes as C

        import numpy as np

        from .capi import check, lib

        tot, per = C.c_double(), np.zeros(self.levels)
        check(lib.pmg_mgmc_get_algorithmic_bytes(self._h, C.byref(tot), per.ctypes.data))
        return tot.value, per

    def set_lowrank(self, B_owned, S):
        """MATLRC fine operator A + B diag(S) B^T, propagated to every level with the hierarchy's own restriction
        (reference src/pc_gamgmc.c:157-196): B_owned = this rank's rows of B (n_owned x k).  Before setup()."""
        import numpy as np

        from .capi import check, lib

        B = np.asarray(B_owned, np.float64)
        S = np.ascontiguousarray(S, np.float64)
        assert B.shape == (self.n_owned, len(S))
        Bl = np.zeros((self.n_local, len(S)), order="F")
        Bl[: self.n_owned] = B
        check(lib.pmg_mgmc_set_lowrank(self._h, len(S), Bl.ctypes.data, S.ctypes.data))

    def setup(self):
        import ctypes as C

        from .capi import check, lib

        err = None
        try:
            check(lib.pmg_mgmc_setup(self._h))
        except Exception as e:  # noqa: BLE001
            err = e
        _all_ok(err, self._group, "row-block hierarchy set-up")
        lib.pmg_rbh_destroy(C.byref(self._rbh))  # the arrays were borrowed until set-up
        return self

    def sample(self, b_owned, y_owned, its: int, seed: int, counter0: int = 0, guesszero: bool = False) -> int:
        """`its` samples; b_owned, y_owned: this rank's rows of the finest level (device tensors, y updated in place).  The
        hierarchy's vectors have one entry per LOCAL row of the finest level (ghost entries ignored)."""
        import ctypes as C

        import torch

        from .capi import check, lib
        from .wrappers import _ptr, _stream

        b = torch.zeros(self.n_local, dtype=torch.float64, device="cuda")
        y = torch.zeros(self.n_local, dtype=torch.float64, device="cuda")
        b[: self.n_owned] = b_owned
        y[: self.n_owned] = y_owned
        out = C.c_uint64()
        check(lib.pmg_mgmc_sample(self._h, _ptr(b), _ptr(y), its, int(guesszero), seed, counter0, C.byref(out), None, None, _stream()))
        y_owned.copy_(y[: self.n_owned])
        return out.value

    def destroy(self):
        import ctypes as C

        from .capi import lib

        if getattr(self, "_h", None):
            lib.pmg_mgmc_destroy(C.byref(self._h))
        if getattr(self, "_rbh", None):  # no set-up ran
            lib.pmg_rbh_destroy(C.byref(self._rbh))


class DistMCSOR:
    """mcgibbs / sorgibbs sampler for an assembled MATAIJ matrix distributed by ROW BLOCKS over `world` ranks
    (reference MCSORApply_MPIAIJ, src/mc_sor.c:298-381: for every colour, update the ghost values, then sweep the
    colour's rows; scatter plan as MatCreateScatters :152-214, de-duplicated per ghost column).

    This rank owns rows [row0, row1) of the global matrix: rowptr / colidx / vals are its rows with GLOBAL column
    indices, colors its rows' entries of a globally valid distance-1 colouring (ncolors colours).  The off-process
    columns become ghost rows (identity rows in an extra colour that is never swept) of a local sliced-ELL operator;
    the per-colour sweeps run on the device (pmg_mcsor_sweep_color_layout), the ghost values travel through
    torch.distributed point-to-point messages between them.  Noise is keyed on the global row, entries keep the order
    of the global CSR row: the chain is the single-process chain bit for bit."""

    def __init__(self, rowptr, colidx, vals, row0, row1, n_global, colors, ncolors, rank, world, omega=1.0, sweep_type=SOR_FORWARD_SWEEP, scaled=True, group=None, transport=None):
        import os

        import numpy as np
        import torch
        import torch.distributed as dist

        from .wrappers import MCSOR

        self.rank, self.world, self.group = rank, world, group
        self.row0, self.row1, self.nloc, self.ncolors = row0, row1, row1 - row0, ncolors
        self.sweep_type, self.scaled = sweep_type, scaled
        rp = np.asarray(rowptr, np.int64)
        ci = np.ascontiguousarray(colidx, np.int64)
        v = np.asarray(vals, np.float64)
        assert len(rp) == self.nloc + 1 and len(colors) == self.nloc
        # --- ghosts and scatter plan (pmg_rowblock.c): who owns my ghosts, what do the others need from me, in which colour
        # does it change -- per colour one gather buffer, the ranks' blocks in rank order
        ranges = [None] * world
        dist.all_gather_object(ranges, (row0, row1), group=group)
        starts = np.array([r[0] for r in ranges] + [n_global], np.int64)
        self.ghosts, plan = _c_rowblock_plan(rank, world, group, starts, ci, colors, ncolors)  # sorted global ids of the ghost columns
        self._plan = plan
        ng = len(self.ghosts)
        is_ghost = (ci < row0) | (ci >= row1)
        loc = np.where(is_ghost, self.nloc + np.searchsorted(self.ghosts, ci), ci - row0)
        # local operator: my rows (entries in the order of the global CSR row) + one identity row per ghost column
        rp2 = np.concatenate([rp, rp[-1] + 1 + np.arange(ng)]).astype(np.int32)
        ci2 = np.concatenate([loc, self.nloc + np.arange(ng)]).astype(np.int32)
        v2 = np.concatenate([v, np.ones(ng)])
        col2 = np.concatenate([np.asarray(colors, np.int32), np.full(ng, ncolors, np.int32)])
        self.mc = MCSOR(rp2, ci2, v2, user_colors=col2)
        self.mc.set_omega(omega)
        self.mc.setup()
        self.mc.set_noise_row_offset(row0)
        pos = self.mc.get_layout().astype(np.int64)
        self.ld = self.mc.layout_len()
        self.pos_local = torch.as_tensor(pos[: self.nloc], device="cuda")
        self._staged = dist.get_backend(group) != "nccl"  # gloo: through host memory
        # --- the C driver (pmg_distmcsor.c): colour sweeps and ghost updates in one C loop on the stream, the updates as
        # one all-gather of the colour's boundary values over the "ipc" or "rccl" transport of pmg_dist.c.  transport
        # "torch" (or none available) keeps the Python loop over torch.distributed point-to-point messages below.
        self._c, self._drv, self.transport = None, None, "none" if world == 1 else "torch"
        want_tr = transport or os.environ.get("PMG_DIST_TRANSPORT")
        if world > 1 and want_tr != "torch":
            on_gpu = dist.get_backend(group) == "nccl"
            drv, name = _agree_on_driver([want_tr] if want_tr else (["ipc", "rccl"] if on_gpu else []), lambda cand: SlabDriver(cand, None, rank, world, group), rank, world, group, "row-block sampler")
            if drv is not None:
                self._drv, self.transport = drv, name
        send_ptr, counts, recv_ptr, recv_src = plan["send_ptr"], plan["counts"], plan["recv_ptr"], plan["recv_src"]
        send_pos, recv_pos = pos[plan["send_rows"]], pos[plan["recv_rows"]]  # layout positions of the plan's local rows
        # --- the point-to-point form of the same plan (exchange(); kept beside the C driver too): a ghost's index in the
        # colour's gather buffer falls into its owner's block (prefix sums of counts[c]); its offset in that block is its
        # index in the owner's send list of the colour.
        # The plan lists ghosts per colour and owner by ascending global row: the order the messages carry.
        offs = np.concatenate([np.zeros((ncolors, 1), np.int64), np.cumsum(counts, axis=1)], axis=1)
        self.send, self.recv = [], []  # per colour: list of (peer, positions in my layout vector)
        reads = [[None] * ncolors for _ in range(world)]  # reads[p][c] = the indices of p's colour-c send list I read
        for c in range(ncolors):
            sl = slice(recv_ptr[c], recv_ptr[c + 1])
            src = recv_src[sl].astype(np.int64)
            peer = np.searchsorted(offs[c], src, side="right") - 1
            self.recv.append([(p, torch.as_tensor(recv_pos[sl][peer == p], device="cuda")) for p in range(world) if (peer == p).any()])
            for p in range(world):
                reads[p][c] = src[peer == p] - offs[c, p]
        wanted = [None] * world
        dist.all_gather_object(wanted, reads, group=group)  # wanted[q][rank][c] = what rank q reads of my colour-c send list
        for c in range(ncolors):
            mine = send_pos[send_ptr[c]:send_ptr[c + 1]]
            self.send.append([(q, torch.as_tensor(mine[wanted[q][rank][c]], device="cuda")) for q in range(world) if q != rank and len(wanted[q][rank][c])])
        if self._drv is not None:
            import ctypes as C

            from .capi import check, lib

            send_pos, recv_pos = send_pos.astype(np.int32), recv_pos.astype(np.int32)
            self._c = C.c_void_p()
            check(lib.pmg_distmcsor_create(self.mc._h, self._drv._h, ncolors, send_ptr.ctypes.data, send_pos.ctypes.data, counts.ctypes.data, recv_ptr.ctypes.data, recv_src.ctypes.data, recv_pos.ctypes.data, C.byref(self._c)))

    def set_lowrank(self, B_owned, S):
        """MATLRC operator A + B diag(S) B^T (reference MCSORSetUp's LRC branch, src/mc_sor.c:572-595): B_owned = this
        rank's rows of B (nloc x k).  C driver only (transport "ipc" / "rccl"); collective."""
        import numpy as np

        from .capi import check, lib

        if self._c is None:
            raise RuntimeError("the low-rank update of the row-block sampler needs the C driver (transport 'ipc' or 'rccl')")
        B = np.asarray(B_owned, np.float64)
        S = np.ascontiguousarray(S, np.float64)
        assert B.shape == (self.nloc, len(S))
        nl = self.nloc + len(self.ghosts)
        Bl = np.zeros((nl, len(S)), order="F")
        Bl[: self.nloc] = B
        check(lib.pmg_distmcsor_set_lowrank(self._c, len(S), nl, self.nloc, Bl.ctypes.data, S.ctypes.data))

    def new_layout(self):
        import torch

        return torch.zeros(self.ld, dtype=torch.float64, device="cuda")

    def to_layout(self, nat_local, out=None):
        out = self.new_layout() if out is None else out
        out[self.pos_local] = nat_local
        return out

    def from_layout(self, lay):
        return lay[self.pos_local]

    def exchange(self, y, color: int):
        """ghost update for the rows of one colour (VecScatterBegin/End of src/mc_sor.c:318-319)"""
        import torch
        import torch.distributed as dist

        ops, bufs = [], []
        for p, idx in self.send[color]:
            t = y[idx]
            t = t.cpu() if self._staged else t
            ops.append(dist.P2POp(dist.isend, t, p, self.group))
        for p, idx in self.recv[color]:
            t = torch.empty(len(idx), dtype=torch.float64, device="cpu" if self._staged else "cuda")
            bufs.append((idx, t))
            ops.append(dist.P2POp(dist.irecv, t, p, self.group))
        if ops:
            for r in dist.batch_isend_irecv(ops):
                r.wait()
        for idx, t in bufs:
            y[idx] = t.cuda() if self._staged else t

    def sample_layout(self, b, y, its: int, seed: int, counter0: int = 0) -> int:
        """`its` samples on layout vectors (b: my rows filled, y: my rows filled; ghost entries are refreshed here)"""
        if self._c is not None:  # the C loop: no Python between colours
            import ctypes as C

            from .capi import check, lib
            from .wrappers import _ptr, _stream

            out = C.c_uint64()
            check(lib.pmg_distmcsor_sample_layout(self._c, _ptr(b), _ptr(y), its, int(self.scaled), self.sweep_type, seed, counter0, C.byref(out), _stream()))
            return out.value
        for c in range(self.ncolors):
            self.exchange(y, c)
        ctr = counter0
        for _ in range(its):
            for direction in directions(self.sweep_type):
                order = range(self.ncolors) if direction == SOR_FORWARD_SWEEP else range(self.ncolors - 1, -1, -1)
                for c in order:
                    self.mc.sweep_color_layout(c, b, y, True, self.scaled, seed, ctr)
                    self.exchange(y, c)
                ctr += 1
        return ctr

    def destroy(self):
        if self._c is not None:
            import ctypes as C

            from .capi import lib

            lib.pmg_distmcsor_destroy(C.byref(self._c))
            self._c = None
        if self._drv is not None:
            self._drv.destroy()
        self._drv = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class DistAIJMGMC(_RowBlockMGMC):
    """MGMC sampler on a caller-supplied hierarchy of assembled MATAIJ matrices distributed by ROW BLOCKS, one rank per
    device: the reference's PCGAMGMC on a MATMPIAIJ (src/pc_gamgmc.c:157-223; level sampler MCSORApply_MPIAIJ,
    src/mc_sor.c:298-381).  `operators[l]` = global CSR triple of level l (0 = coarsest), `interpolations[l]` (l >= 1) =
    global CSR triple of the prolongation from level l-1 to level l -- what MGMC.from_hierarchy takes, available on every
    rank; `starts[l]` = the world+1 row-block boundaries of level l (default: equal blocks).  Every rank keeps its rows of
    the levels with more than `replicate_below` rows (plus one ghost row per row of another rank that its operator,
    restriction or the finer level's interpolation reads) and the WHOLE of the smaller levels -- at least the coarsest,
    which is factored redundantly: there every rank runs the single-device kernels on identical data, which costs less
    than a ghost update per colour for a few thousand rows.  The whole sample loop -- colour
    sweeps, ghost updates, residuals, transfers, coarse solve -- runs in C (pmg_mgmc.c) on the stream; this class only
    agrees on a transport and slices the matrices, the rest is _RowBlockMGMC: the set-up of pmg_rowblock.c (pmg_rbh_*;
    host code, collective) that CRowBlock.mgmc and the adapter reach too.  Bit-identical to MGMC.from_hierarchy."""

    def __init__(self, operators, interpolations, rank: int, world: int, group=None, transport=None, starts=None, replicate_below: int = 50000, coloring: int = 0):
        import os

        import numpy as np

        self.rank, self.world, self.group = rank, world, group
        L = len(operators)
        assert L >= 2 and len(interpolations) == L
        n = [len(op[0]) - 1 for op in operators]
        # --- transport: the generic all-gather of pmg_dist.c ("ipc" peer stores or RCCL), agreed between the ranks
        want_tr = transport or os.environ.get("PMG_DIST_TRANSPORT")
        self._drv, self.transport = _agree_on_driver([want_tr] if want_tr else ["ipc", "rccl"], lambda cand: SlabDriver(cand, None, rank, world, group), rank, world, group, "row-block hierarchy")
        if self._drv is None:
            raise RuntimeError("DistAIJMGMC needs the 'ipc' or 'rccl' transport of the HIP library")
        # --- this rank's rows of every level, global columns, entries in the caller's order (the summation order of a row);
        # fold, colouring (the rule MGMC.from_hierarchy + set_coloring(rule) sweeps with on one device), restriction rows,
        # ghost plans and local matrices are pmg_rowblock.c's
        if starts is None:
            starts = [np.linspace(0, n[l], world + 1).astype(np.int64) for l in range(L)]

        def rows(triple, r0, r1):
            rp, ci, v = (np.asarray(a_) for a_ in triple)
            return rp[r0:r1 + 1] - rp[r0], ci[rp[r0]:rp[r1]], v[rp[r0]:rp[r1]]

        cut = [(int(starts[l][rank]), int(starts[l][rank + 1])) for l in range(L)]
        super().__init__(self._drv, [dict(n=n[l], row0=cut[l][0], A=rows(operators[l], *cut[l]), P=rows(interpolations[l], *cut[l]) if l >= 1 else None) for l in range(L)], replicate_below, coloring)

    def destroy(self):
        super().destroy()
        if getattr(self, "_drv", None) is not None:
            self._drv.destroy()  # collective: disconnect, barrier, destroy
            self._drv = None


class CRowBlock:
    """The multi-rank samplers on MATMPIAIJ row blocks reached through the C-ABI ALONE (pmg_rowblock.c): transport bootstrap,
    colouring, ghost plans, local operators and the sample loops are C; Python only supplies the byte all-gather callback
    (torch.distributed here, MPI_Allgather in adapter/, pipes in examples/pmg_bench.c) and device tensors.  This is what a
    PETSc caller with an MPI_Comm uses.  DistMCSOR / DistAIJMGMC above take the same transport
    (SlabDriver), the same ghost plans and the same hierarchy (_RowBlockMGMC) from pmg_rowblock.c; they differ in
    who slices the rows (they do, from global matrices every rank holds) and in that they fall back from one transport to
    the next after a self-test (_agree_on_driver), where `transport` here is taken as given.

      CRowBlock.sampler(...)  MCSORCreate + MCSORSetUp + the sample loop on a MATMPIAIJ (reference src/mc_sor.c:298-381,553-605)
      CRowBlock.mgmc(...)     PCGAMGMC on a hierarchy of MATMPIAIJ levels (src/pc_gamgmc.c:157-264)"""

    def __init__(self, rank: int, world: int, group=None, transport: str = "ipc"):
        import ctypes as C

        self.rank, self.world, self.transport = rank, world, transport
        self._drv = SlabDriver(transport, None, rank, world, group)
        self.comm = self._drv._comm[0]
        self._mc, self._dm, self._mg = C.c_void_p(), C.c_void_p(), None
        self.nowned = 0

    @property
    def dist_handle(self):
        return self._drv._h

    def sampler(self, row_starts, rowptr, colidx_global, vals, omega=1.0, colors=None, ncolors=0):
        """this rank's rows with GLOBAL columns (pmg_rowblock_merge_mpiaij of MatMPIAIJGetSeqAIJ's blocks); colors None: the
        library's first-fit colouring of the global matrix"""
        import ctypes as C

        import numpy as np

        from .capi import check, lib

        rs = np.ascontiguousarray(row_starts, np.int64)
        rp, ci, v = np.ascontiguousarray(rowptr, np.int64), np.ascontiguousarray(colidx_global, np.int64), np.ascontiguousarray(vals, np.float64)
        col = None if colors is None else np.ascontiguousarray(colors, np.int32)
        self.nowned = int(rs[self.rank + 1] - rs[self.rank])
        check(lib.pmg_rowblock_sampler_create(C.byref(self.comm), self.dist_handle, rs.ctypes.data, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, 64, ncolors, col.ctypes.data if col is not None else None, omega, C.byref(self._mc), C.byref(self._dm)))
        return self

    def sample(self, b_owned, y_owned, its: int, seed: int, counter0: int = 0, scaled: bool = True, sweep_type: int = SOR_FORWARD_SWEEP) -> int:
        import ctypes as C

        from .capi import check, lib
        from .wrappers import _ptr, _stream

        if self._mg is not None:
            return self._mg.sample(b_owned, y_owned, its, seed, counter0)
        out = C.c_uint64()
        check(lib.pmg_distmcsor_sample(self._dm, self.nowned, _ptr(b_owned), _ptr(y_owned), its, int(scaled), sweep_type, seed, counter0, C.byref(out), _stream()))
        return out.value

    def apply(self, b_owned, y_owned, sweep_type: int = SOR_FORWARD_SWEEP):
        from .capi import check, lib
        from .wrappers import _ptr, _stream

        check(lib.pmg_distmcsor_apply(self._dm, self.nowned, _ptr(b_owned), _ptr(y_owned), sweep_type, _stream()))

    def mgmc(self, levels, replicate_below: int = 50000, smoother=(True, 1.0, SOR_FORWARD_SWEEP, 1), lowrank=None):
        """levels[l] = dict(n=global rows, row0=, A=(rowptr, colidx_global, vals) of this rank's rows, P=(rowptr,
        colidx_global_coarse, vals) of this rank's rows of P_l (l >= 1)); level 0 = coarsest"""
        self._mg = _RowBlockMGMC(self._drv, levels, replicate_below)
        self.nowned, self.nlocal = self._mg.n_owned, self._mg.n_local
        self._mg.set_smoother(*smoother)
        if lowrank is not None:
            self._mg.set_lowrank(*lowrank)
        self._mg.setup()
        return self

    def destroy(self):
        """collective"""
        import ctypes as C

        from .capi import lib

        if self._mg is not None:
            self._mg.destroy()
        if self._dm:
            lib.pmg_distmcsor_destroy(C.byref(self._dm))
        if self._mc:
            lib.pmg_mcsor_destroy(C.byref(self._mc))
        self._drv.destroy()

