"""Row-slab partitioning of the image across ranks and the neighbour halo exchange.

The filter window of a pixel reaches b = (box-1)/2 rows up and down (rpf.cpp:561-571) and nothing else is
shared between pixels, so the image shards into contiguous row slabs, one per GPU / process, and the only
data-path communication is a send/recv of b boundary rows with the rank above and the rank below
(`torch.distributed` P2P: RCCL over xGMI on the GPUs, gloo in the CPU tests).  Feature planes never change
between passes, so their halo is exchanged once; colours change every pass and are re-exchanged before
each pass.  Planes are laid out [plane][row][x][s], so a halo is one contiguous span per plane.

pbrt's film step (rpf_film_splat_device) also runs slab by slab: ``film_halo_rows`` is the halo it needs (the slab takes the
larger of that and b), and after one more colour exchange behind the last pass ``film_for_slab`` describes the rank's buffer
as a sample film of its own whose output rows are the rows the rank owns.  Both are pure geometry: no torch, no GPU.
"""
from collections import namedtuple

Slab = namedtuple("Slab", "row0 row1 halo_top halo_bottom")  # owned image rows [row0,row1); halo rows held


def partition_rows(H, world, rank):
    """contiguous, near-equal split of H rows: rank r owns [r*H//world, (r+1)*H//world)"""
    return (rank * H) // world, ((rank + 1) * H) // world


def slab_for(H, world, rank, halo):
    """rank's slab; every rank must own at least `halo` rows, because a neighbour's halo is filled from this rank's
    OWNED boundary rows only (a thinner slab would have to forward rows it does not own)"""
    a, b = partition_rows(H, world, rank)
    if world > 1 and b - a < halo:
        raise ValueError("row slab of rank %d has %d rows, fewer than the %d halo rows its neighbours need: "
                         "use fewer ranks (H = %d, world = %d)" % (rank, b - a, halo, H, world))
    return Slab(a, b, min(halo, a), min(halo, H - b))


def buffer_rows(slab):
    """rows present in the rank's buffers, and the [row_begin,row_end) range the rank filters"""
    n = slab.row1 - slab.row0
    return slab.halo_top + n + slab.halo_bottom, slab.halo_top, slab.halo_top + n


def check_desc(desc):
    """Refuses a descriptor these helpers cannot drive yet.  SAMPLED_NBHD_FLAG: a sampled pass keys every pixel by its IMAGE row
    and by the pass id, so a rank would have to set ``Sampling.row_origin`` to its buffer's first image row and ``pass_id0`` to
    the pass of each one-pass call; nothing here does, and a rank that filtered with the whole
    image's configuration would silently draw other samples than the whole image does.  MEMBER_TEST_FLAG: every rank's context
    would need the same ``set_membership`` and these helpers carry no such configuration; the test itself is a function of the
    pixel alone, so MultiContext (or a caller that configures each rank's context) gives the whole image's bits.  SCHEDULE_FLAG:
    every rank's context would need the same ``set_schedule`` and, since these helpers drive one pass per call, a ``pass0`` that
    moves with each call; nothing here does either.  PASS_REPORT_FLAG: a rank's one-pass calls each fill entry 0 of its own
    context, and the merged report needs every rank's row records gathered in image-row order; nothing here gathers them."""
    from . import hip
    if desc.flags & hip.SAMPLED_NBHD_FLAG:
        raise NotImplementedError("slabs: SAMPLED_NBHD_FLAG (RPF_FLAG_SAMPLED_NBHD) is not supported across ranks yet: each rank must set "
                                  "Sampling.row_origin (image row of its buffer row 0) and pass_id0 per one-pass call itself "
                                  "(INTEGRATION.md section 2f), or use MultiContext, which does")
    if desc.flags & hip.MEMBER_TEST_FLAG:
        raise NotImplementedError("slabs: MEMBER_TEST_FLAG (RPF_FLAG_MEMBER_TEST) is not supported across ranks yet: each rank's context "
                                  "needs the same Context.set_membership, which these helpers do not carry (INTEGRATION.md "
                                  "section 2g), or use MultiContext, which does")
    if desc.flags & hip.SCHEDULE_FLAG:
        raise NotImplementedError("slabs: SCHEDULE_FLAG (RPF_FLAG_SCHEDULE) is not supported across ranks yet: each rank's context needs "
                                  "the same Context.set_schedule table and, for these one-pass calls, Schedule.pass0 set to the pass "
                                  "of each call (INTEGRATION.md section 2h), or use MultiContext, which does")
    if desc.flags & hip.PASS_REPORT_FLAG:
        raise NotImplementedError("slabs: PASS_REPORT_FLAG (RPF_FLAG_PASS_REPORT) is not supported across ranks yet: each rank would "
                                  "report its own rows as entry 0 of every one-pass call, and nothing here gathers the row records "
                                  "in image-row order for hip.pass_report_fold (INTEGRATION.md section 2i), or use MultiContext, "
                                  "which does")
    return desc


def film_halo_rows(desc, film):
    """rows of each neighbour a slab must hold for the film step: the gather's row half-width for the WHOLE image
    (rpf_film_window; desc and film describe the whole sample film).  ``slab_for`` is called with the larger of this and
    the box halo."""
    from . import hip
    return hip.film_window(check_desc(desc), film)[1]


def film_for_slab(film, slab, H):
    """The film step of one rank.  Returns (a copy of ``film`` that describes the rank's buffer as a sample film of its
    own, (r0, r1)): ``sample_y0`` is moved to the buffer's first image row and the output rows [py0, py1) are clipped to
    the rows the rank owns (the first / last rank also takes the output rows above / below the sample film); r0, r1 are
    the rows of the whole-image outputs [py1 - py0][px1 - px0] that the rank's outputs fill.  None when the rank owns no
    output row (a crop window elsewhere).  H = rows of the whole sample film.  Every output pixel then gathers the same
    samples in the same order as in the whole frame, provided the slab holds ``film_halo_rows`` rows of each neighbour
    and their colours were exchanged after the last pass."""
    y_own0 = film.sample_y0 + slab.row0
    y_own1 = film.sample_y0 + slab.row1
    oy0 = film.py0 if slab.row0 == 0 else max(film.py0, y_own0)
    oy1 = film.py1 if slab.row1 == H else min(film.py1, y_own1)
    if oy1 <= oy0:
        return None
    f = type(film).from_buffer_copy(film)
    f.sample_y0 = film.sample_y0 + slab.row0 - slab.halo_top
    f.py0, f.py1 = oy0, oy1
    return f, (oy0 - film.py0, oy1 - film.py0)


def exchange_halo(t, slab, rank, world, group=None):
    """Refresh the halo rows of ``t`` ([planes, H_buf, W, S], any dtype) from the neighbouring ranks' owned
    boundary rows.  Collective over (rank-1, rank, rank+1); a no-op for world == 1."""
    import torch.distributed as dist
    if world == 1:
        return
    n_own = slab.row1 - slab.row0
    top0 = slab.halo_top  # first owned buffer row
    assert n_own >= max(slab.halo_top, slab.halo_bottom), "slab thinner than its halo (see slab_for)"
    ops, recvs = [], []
    # gloo moves host memory only: device tensors are staged through the host (CPU tests, single-GPU rehearsals of the
    # multi-rank path); nccl (= RCCL) sends device memory directly over xGMI
    stage = t.is_cuda and dist.get_backend(group) == "gloo"
    wire = (lambda x: x.cpu()) if stage else (lambda x: x)
    if rank > 0 and slab.halo_top > 0:
        h = slab.halo_top
        send_up = wire(t[:, top0:top0 + h].contiguous())    # my first h owned rows -> bottom halo of rank-1
        recv_up = wire(t.new_empty((t.shape[0], h) + tuple(t.shape[2:])))
        ops += [dist.P2POp(dist.isend, send_up, rank - 1, group), dist.P2POp(dist.irecv, recv_up, rank - 1, group)]
        recvs.append((recv_up, 0, h))
    if rank < world - 1 and slab.halo_bottom > 0:
        h = slab.halo_bottom
        send_dn = wire(t[:, top0 + n_own - h:top0 + n_own].contiguous())  # my last h owned rows -> top halo of rank+1
        recv_dn = wire(t.new_empty((t.shape[0], h) + tuple(t.shape[2:])))
        ops += [dist.P2POp(dist.isend, send_dn, rank + 1, group), dist.P2POp(dist.irecv, recv_dn, rank + 1, group)]
        recvs.append((recv_dn, top0 + n_own, h))
    if ops:
        for req in dist.batch_isend_irecv(ops):
            req.wait()
    for buf, r0, h in recvs:
        t[:, r0:r0 + h].copy_(buf)  # (host -> device when staged)


class HaloPlan:
    """exchange_halo() with its send / receive staging buffers allocated once (nothing is allocated inside a timed
    loop): ``plan = HaloPlan(t, slab, rank, world)``, then ``plan.exchange(t)`` before every pass."""

    def __init__(self, t, slab, rank, world, group=None):
        import torch.distributed as dist
        self.slab, self.rank, self.world, self.group = slab, rank, world, group
        self.stage = world > 1 and t.is_cuda and dist.get_backend(group) == "gloo"
        n_own = slab.row1 - slab.row0
        assert world == 1 or n_own >= max(slab.halo_top, slab.halo_bottom), "slab thinner than its halo (see slab_for)"

        def buf(h):
            shape = (t.shape[0], h) + tuple(t.shape[2:])
            return t.new_empty(shape, device="cpu") if self.stage else t.new_empty(shape)

        self.up = (buf(slab.halo_top), buf(slab.halo_top)) if world > 1 and rank > 0 and slab.halo_top > 0 else None
        self.dn = (buf(slab.halo_bottom), buf(slab.halo_bottom)) if world > 1 and rank < world - 1 and slab.halo_bottom > 0 else None

    def exchange(self, t):
        if self.world == 1:
            return
        import torch.distributed as dist
        slab, rank, group = self.slab, self.rank, self.group
        n_own, top0 = slab.row1 - slab.row0, slab.halo_top
        ops = []
        if self.up is not None:
            h = slab.halo_top
            self.up[0].copy_(t[:, top0:top0 + h])                       # my first h owned rows -> bottom halo of rank-1
            ops += [dist.P2POp(dist.isend, self.up[0], rank - 1, group), dist.P2POp(dist.irecv, self.up[1], rank - 1, group)]
        if self.dn is not None:
            h = slab.halo_bottom
            self.dn[0].copy_(t[:, top0 + n_own - h:top0 + n_own])       # my last h owned rows -> top halo of rank+1
            ops += [dist.P2POp(dist.isend, self.dn[0], rank + 1, group), dist.P2POp(dist.irecv, self.dn[1], rank + 1, group)]
        if ops:
            for req in dist.batch_isend_irecv(ops):
                req.wait()
        if self.up is not None:
            t[:, 0:slab.halo_top].copy_(self.up[1])
        if self.dn is not None:
            t[:, top0 + n_own:top0 + n_own + slab.halo_bottom].copy_(self.dn[1])
