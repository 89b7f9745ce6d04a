"""Index-bit-partitioned statevector across the GPUs of one node (one process per GPU, RCCL over xGMI
through ``torch.distributed`` — backend "nccl" IS RCCL on ROCm; "gloo" in the CPU tests).

Layout: W = 2^g ranks, rank r owns the 2^(n-g) amplitudes whose PHYSICAL index has r in its top g bits.
A logical->physical bit permutation is tracked, so "which logical qubits are global" is a planner
decision, not a fixed property of the register.

Per Pauli rotation exp(-i phi P), P = (x, z):
  * z on a global bit  -> a rank-dependent sign inside the local kernel, zero traffic;
  * x only on local bits -> the local HIP sweep of libovqe_sv (shard handle, ``ovqe_create_shard``);
  * x on a global bit  -> that logical qubit is first made local by a SHARD EXCHANGE: k global physical
    bits are traded for k local ones in one all-to-all among the 2^k ranks of a sub-cube — every rank
    keeps 1/2^k of its shard and sends S/2^k to each of its 2^k - 1 partners, each over its own xGMI
    link (k = 1: the half-shard exchange with one partner, S/2 over one link) —, packed and unpacked by
    the shard handle's kernels (``ovqe_shard_pack`` / ``ovqe_shard_unpack``), after which the rotation
    is local.  The exchange is NOT undone: the permutation is updated instead, and the qubits sent away
    are chosen Belady-style (farthest next X/Y use), so a run of rotations touching the same qubits pays
    for one exchange only; because a larger exchange is cheaper per link, it also brings in every global
    qubit that is needed sooner than a local one it can send away (``max_exchange_bits``).

Expectation values: Hamiltonian terms are grouped by the global part of their x mask; the x_g = 0 group
is a local partial sum; the <= 2^g - 1 other groups read their partner's shard in CHUNKS (2^26 amplitudes =
1 GiB by default): chunk c of ALL partners is received as one batch — every xGMI link of the group list
busy at once — double-buffered against the contraction of chunk c - 1 (2 x 7 x 1 GiB instead of two
whole shards), and ``ovqe_bilinear`` on an m-bit sub-register contracts the matching chunk of the own
shard (bra) with the received chunk (ket), the index bits above the chunk folded into the coefficients
on the host; one scalar all-reduce at the end.
The ADAPT gradient screen shards the same way (``apply_hamiltonian`` builds the sigma shard group by
group, ``pool_gradients`` contracts the pool per partner shard in one batched launch each, one
all-reduce of the pool-sized result).  Exchanges travel in pipelined pieces.  No other
collective exists on the data path.

Exact gradient (``program_energy_gradient``): the adjoint method on shards — forward plan, lambda = H psi sharded like psi,
then the plan's steps in reverse on psi AND lambda: a rotation step is one ``ovqe_adjoint_rotations`` call per shard (local
sums w_r, both vectors un-rotated), an exchange step the same k-bit exchange for both vectors (a swap of disjoint bit pairs is
its own inverse); one all-reduce of the R sums at the end.
"""
from __future__ import annotations

import time

import numpy as np
import torch
import torch.distributed as dist


class DistWatchdog:
    """Deadline over the collective waits of a multi-rank run.  RCCL's `Work.wait()` only orders streams and the stream
    synchronisation that follows cannot time out, so a rank whose partner never posts its half of an exchange would sit there
    until somebody kills the job.  A daemon thread checks a deadline that every progress point of the sharded register
    (`kick`: each half-shard exchange, each chunk of a partner read, each all-reduce) pushes `timeout_s` into the future; when
    it passes, `on_expire(phase, seconds)` runs on that thread (the blocked main thread has released the GIL inside the wait)
    and the process leaves with `exit_code` through `os._exit` — no exec, no clean-up that could block again.
    `OVQE_DIST_TIMEOUT_S` (default 120) sets the time."""

    def __init__(self, on_expire=None, timeout_s=None, exit_code=3):
        import os
        import threading
        self.timeout_s = float(os.environ.get("OVQE_DIST_TIMEOUT_S", "120")) if timeout_s is None else float(timeout_s)
        self.on_expire = on_expire
        self.exit_code = exit_code
        self.phase = "start"
        self.expired = False
        self._deadline = time.monotonic() + self.timeout_s
        self._stop = threading.Event()
        self._thread = threading.Thread(target=self._run, name="ovqe-dist-watchdog", daemon=True)
        self._thread.start()

    def kick(self, phase=None):
        if phase is not None:
            self.phase = phase
        self._deadline = time.monotonic() + self.timeout_s

    def stop(self):
        self._stop.set()

    def _run(self):
        import os
        while not self._stop.wait(min(0.25, self.timeout_s / 4)):
            late = time.monotonic() - self._deadline
            if late > 0:
                self.expired = True
                try:
                    if self.on_expire is not None:
                        self.on_expire(self.phase, self.timeout_s + late)
                finally:
                    if self.exit_code is not None:
                        os._exit(self.exit_code)
                return


#: the watchdog of this process, if the launcher installed one (bench.py does for every multi-rank run)
watchdog = None


def _progress(phase=None):
    if watchdog is not None:
        watchdog.kick(phase)


def permute_mask(mask, perm):
    out = 0
    m = int(mask)
    b = 0
    while m:
        if m & 1:
            out |= 1 << perm[b]
        m >>= 1
        b += 1
    return out


class HipShardEngine:
    """Shard-local compute on one MI355X through the C ABI; the state buffer is a torch tensor so that
    torch.distributed can send/receive slices of it."""

    def __init__(self, n_local, n_global, rank, device):
        from .backend import Statevector
        self.device = torch.device("cuda", device)
        self.tensor = torch.zeros(1 << n_local, dtype=torch.complex128, device=self.device)
        self.sv = Statevector(n_local, device=device, n_global=n_global, shard_index=rank)
        self.sv.adopt_state(self.tensor.data_ptr())
        # RCCL's Work.wait() orders torch's CURRENT stream behind a transfer, nothing else: the handle's kernels must run
        # on that very stream, or a contraction could read a partner shard before it has arrived
        self.stream = torch.cuda.current_stream(self.device)
        self.sv.set_stream(self.stream.cuda_stream)
        self._subs = {}
        # what the local kernels really did: passes over the shard (launches that stream it) and the bytes they move by
        # construction — fused same-x runs and LDS-tiled multi-run sweeps make this smaller than one sweep per rotation
        self.counters = {"rotations": 0, "rotation_passes": 0, "rotation_bytes": 0, "contraction_calls": 0, "contraction_passes": 0,
                         "contraction_bytes": 0, "adjoint_passes": 0, "adjoint_bytes": 0, "pool_plans": 0}

    def check_stream(self):
        if torch.cuda.current_stream(self.device).cuda_stream != self.stream.cuda_stream:
            raise RuntimeError("ShardedStatevector was created under another torch stream: its shard kernels would not be "
                               "ordered behind RCCL transfers waited for on this one")

    def new_buffer(self, count, dtype=None):
        """scratch of ``count`` amplitudes in the shard's current storage (complex128, or float64 under real storage)"""
        return torch.empty(count, dtype=self.tensor.dtype if dtype is None else dtype, device=self.device)

    @property
    def is_real(self):
        return self.tensor.dtype == torch.float64

    def set_real(self, flag, discard=False):
        """Storage of the shard: 2^n_local complex128 (16 B) or — while every applied rotation keeps a real state real — float64
        (8 B: half the HBM bytes of every sweep, of <H> and of every transfer; option "real_state" of the handle).  The amplitudes
        are converted unless ``discard`` (an initialisation follows)."""
        flag = bool(flag)
        if flag == self.is_real:
            return
        size = self.tensor.numel()
        if discard:
            self.tensor = None
            new = torch.zeros(size, dtype=torch.float64 if flag else torch.complex128, device=self.device)
        elif flag:
            new = torch.view_as_real(self.tensor)[:, 0].contiguous()
        else:
            new = torch.complex(self.tensor, torch.zeros_like(self.tensor))
        self.sync()
        self.tensor = new
        self.sv.adopt_state(new.data_ptr())
        self.sv.set_option("real_state", 1 if flag else 0)
        for sub in self._subs.values():
            sub.close()
        self._subs = {}

    def sync(self):
        torch.cuda.synchronize(self.device)

    def init_basis(self, global_index):
        self.sv.init_basis(global_index)

    def randomize(self, seed, norm2_total=0.0):
        return self.sv.randomize(seed, norm2_total)

    def norm2(self):
        return self.sv.norm2()

    def _count(self, what, sv, calls=1):
        passes, nbytes = sv.last_passes()
        self.counters[what + "_passes"] += passes
        self.counters[what + "_bytes"] += nbytes
        self.counters["rotations" if what == "rotation" else "contraction_calls"] += calls

    def rotations(self, xs, zs, phis):
        self.sv.apply_pauli_rotations(xs, zs, phis)
        self._count("rotation", self.sv, len(xs))

    def adjoint_rotations(self, lam, xs, zs, phis):
        """backward step of the adjoint method on the shard and on ``lam`` (a shard-sized complex buffer): the rotations are
        un-applied last to first from both -> the local sums w[r] = Im <lam|P_r|psi> (``ovqe_adjoint_rotations``)"""
        w = self.sv.adjoint_rotations(lam.data_ptr(), xs, zs, phis)
        passes, nbytes = self.sv.last_passes()
        self.counters["adjoint_passes"] += passes
        self.counters["adjoint_bytes"] += nbytes
        return w

    def set_tensor(self, tensor):
        """make another shard-sized buffer of the shard's storage the shard the handle works on (the exchange of lambda in the backward
        pass: pack / unpack read and write the handle's state; the rotating vectors of the Lanczos recurrence: sigma = H psi reads
        the handle's state); the previous buffer stays with the caller"""
        if tensor.dtype != self.tensor.dtype or tensor.numel() != self.tensor.numel():
            raise ValueError("set_tensor: a buffer of the shard's size in the shard's storage (complex128, or float64 on a real shard)")
        self.sync()
        self.tensor = tensor
        self.sv.adopt_state(tensor.data_ptr())

    def bilinear_batch(self, offsets, xs, zs, coeffs, bra, ket=None):
        return self.sv.bilinear_batch(offsets, xs, zs, coeffs, bra_ptr=bra.data_ptr(),
                                      ket_ptr=None if ket is None else ket.data_ptr())

    # -- k-bit exchange: block ``block`` of the local bits ``mask`` <-> a contiguous stream of the shard's elements (or of the real parts
    # of a complex shard); positions [first, first + count) of the block; only enqueued on the engine's stream
    def pack(self, mask, block, first, count, dst, real_parts_only=False):
        self.sv.shard_pack(mask, block, first, count, dst.data_ptr(), real_parts_only)

    def unpack(self, mask, block, first, count, src, real_parts_only=False):
        self.sv.shard_unpack(mask, block, first, count, src.data_ptr(), real_parts_only)

    # -- Pauli sums planned once per (Hamiltonian, permutation): ovqe_xsum_* (csrc/cross_host.inc, csrc/sv_cross.hpp).  Masks in the
    # physical bit space of the whole register; the remote calls only enqueue kernels on the engine's stream
    def plan_sum(self, xs, zs, coeffs, chunk_bits):
        return self.sv.xsum_create(xs, zs, coeffs, chunk_bits)

    def free_sum(self, sid):
        self.sv.xsum_destroy(sid)

    def sum_info(self, sid):
        return self.sv.xsum_info(sid)

    def sum_partners(self, sid):
        return self.sv.xsum_partners(sid)

    def sum_expect_local(self, sid):
        out = self.sv.xsum_expect_local(sid)
        self._count("contraction", self.sv)
        return out

    def sum_expect_remote(self, sid, d, chunk, ket):
        self.sv.xsum_expect_remote(sid, d, chunk, ket.data_ptr())
        self._count("contraction", self.sv)

    def sum_expect_finish(self, sid):
        return self.sv.xsum_expect_finish(sid)

    def sum_apply_local(self, sid, out, ident=0.0):
        self.sv.xsum_apply_local(sid, out.data_ptr(), ident)

    def sum_apply_remote(self, sid, d, chunk, ket, out):
        self.sv.xsum_apply_remote(sid, d, chunk, ket.data_ptr(), out.data_ptr())

    # -- the ADAPT pool planned once per (pool, permutation, chunk bits): ovqe_xpool_* (csrc/pool_host.inc, csrc/sv_pool.hpp).  Terms in
    # CSR form over the operators, masks in the physical bit space of the whole register; ``bra`` = this rank's sigma shard in the shard's
    # storage; local / remote only enqueue kernels on the engine's stream, finish synchronises
    def plan_pool(self, offsets, xs, zs, coeffs, chunk_bits):
        self.counters["pool_plans"] += 1
        return self.sv.xpool_create(offsets, xs, zs, coeffs, chunk_bits)

    def free_pool(self, pid):
        self.sv.xpool_destroy(pid)

    def pool_info(self, pid):
        return self.sv.xpool_info(pid)

    def pool_partners(self, pid):
        return self.sv.xpool_partners(pid)

    def pool_local(self, pid, bra):
        self.sv.xpool_local(pid, bra.data_ptr())
        self._count("contraction", self.sv)

    def pool_remote(self, pid, d, chunk, ket, bra):
        self.sv.xpool_remote(pid, d, chunk, ket.data_ptr(), bra.data_ptr())
        self._count("contraction", self.sv)

    def pool_finish(self, pid):
        return self.sv.xpool_finish(pid)

    # -- Lanczos vector operations on shard-sized buffers of the shard's storage (ovqe_vec_*): this shard's partial sums; dot and
    # update synchronise, scale and axpy only enqueue on the engine's stream
    def vec_dot(self, a, b):
        return self.sv.vec_dot(a.data_ptr(), b.data_ptr())

    def vec_update(self, w, v, vprev, alpha, beta):
        """w <- w - alpha v - beta vprev (vprev may be None) -> sum |w_i|^2 over this shard"""
        return self.sv.vec_lanczos_update(w.data_ptr(), v.data_ptr(), None if vprev is None else vprev.data_ptr(), alpha, beta)

    def vec_scale(self, v, s):
        self.sv.vec_scale(v.data_ptr(), s)

    def vec_axpy(self, y, x, s, overwrite=False):
        self.sv.vec_axpy(y.data_ptr(), x.data_ptr(), s, overwrite)

    # -- the pool contraction on CHUNKS: 2^m consecutive amplitudes of a shard-sized buffer against a received chunk of the
    # partner's shard; masks live on the m low bits (the host layer folds everything above them into the coefficients)
    def _sub(self, m):
        if m not in self._subs:
            from .backend import Statevector
            # (never used as a state — bra and ket pointers come with every call: a view of the shard, no 2^m-amplitude allocation)
            sub = Statevector(m, device=self.device.index, view_of=self.tensor.data_ptr())
            sub.set_stream(self.stream.cuda_stream)
            self._subs[m] = sub
        return self._subs[m]

    def sub_bilinear_batch(self, m, offsets, xs, zs, coeffs, bra, bra_off, ket):
        return self._sub(m).bilinear_batch(offsets, xs, zs, coeffs, bra_ptr=bra.data_ptr() + 16 * bra_off, ket_ptr=ket.data_ptr())


class ShardedStatevector:
    """n-qubit state over ``dist.get_world_size()`` ranks (a power of two)."""

    def __init__(self, n_qubits, engine_factory=None, group=None, device=None, dry_rank=None):
        """``dry_rank`` = (world, rank): ONE rank of a ``world``-rank register without the others — no process group; a half-shard
        exchange packs, "receives" its own packed half and unpacks, a partner-shard read hands out this rank's own chunks.  The
        amplitudes are then meaningless, but every kernel launch, every pack / unpack copy and every byte that would cross a link
        is what that rank of the real job executes and counts: the per-rank compute time of configs[4] at full shard size, measured
        on one GPU (bench.py ``scale_proxy``)."""
        self.group = group
        self.dry = dry_rank is not None
        if self.dry:
            self.world, self.rank = int(dry_rank[0]), int(dry_rank[1])
        else:
            self.world = dist.get_world_size(group) if dist.is_initialized() else 1
            self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        g = self.world.bit_length() - 1
        if (1 << g) != self.world:
            raise ValueError("world size must be a power of two")
        if n_qubits - g < 1:
            raise ValueError("too few qubits for this many ranks")
        self.n, self.g, self.n_local = int(n_qubits), g, int(n_qubits) - g
        self.perm = list(range(self.n))  # logical index bit -> physical index bit
        if engine_factory is None:
            dev = device if device is not None else torch.cuda.current_device()
            engine_factory = lambda nl, ng, r: HipShardEngine(nl, ng, r, dev)  # noqa: E731
        self.engine = engine_factory(self.n_local, self.g, self.rank)
        self._dist = dist.is_initialized() and not self.dry
        self.stats = {"swaps": 0, "bytes_sent": 0, "full_shard_reads": 0, "chunk_reads": 0, "partners_per_read": 0, "pieces": 0,
                      "swap_s": 0.0, "shard_read_s": 0.0, "real_exchanges": 0, "real_chunk_reads": 0,
                      # exchanges: bytes to ONE partner per exchange, summed (the busiest link: all partners of an exchange are served
                      # at once, each over its own link), and the sum of the bits traded
                      "link_bytes": 0, "exchange_bits": 0,
                      # seconds this rank's kernels ran, by phase (each section ends with a device synchronisation)
                      "local_sweeps_s": 0.0, "expectation_local_s": 0.0, "expectation_remote_s": 0.0, "apply_s": 0.0,
                      "adjoint_sweeps_s": 0.0,
                      # the planned ADAPT screen: seconds of its pool contractions (local, per chunk, finish) and the plans made
                      "screen_s": 0.0, "pool_plans": 0}
        # Several ranks on ONE device (the gloo runs of the tests and of bench.py's single-device mode) would time each other's
        # kernels: with a lock file every compute section takes the device alone (flock), so its seconds are this rank's own
        self.compute_lock = None
        # Most index bits one exchange trades (a k-bit exchange is an all-to-all among 2^k ranks: S/2^k per link instead of S/2).  1:
        # half-shard exchanges only, planned one missing qubit at a time
        import os
        self.max_exchange_bits = max(1, min(max(g, 1), int(os.environ.get("OVQE_EXCHANGE_BITS", max(g, 1)))))
        self._tmp = None
        self._chunk_bufs = None
        self._chunk_real = None
        self._chunk_send = None
        self._sigma = None
        # Real-amplitude transfers: a basis state evolved by rotations whose strings all carry an odd number of Y — every UCC / ADAPT
        # generator (-i phi P is then a real antisymmetric matrix) — has real amplitudes; while that holds, half-shard exchanges and
        # partner-shard reads move the real parts only: 8 instead of 16 bytes per amplitude over xGMI.  (The shard kernels keep their
        # complex layout; the imaginary parts are exact zeros and are rebuilt as such on arrival.)
        self.real = False
        self.real_transfers = True
        # Real STORAGE (engines that offer it: the HIP engine): a compiled program whose strings all have an odd number of Y runs on
        # float64 shards — local sweeps, <H> and transfers on 8-byte amplitudes; anything that needs complex amplitudes (a rotation
        # with an even number of Y, sigma = H psi of a sum that is not real-symmetric, the Taylor series) widens the shard back first
        self.real_storage = True

    # -- helpers ----------------------------------------------------------------------------
    def _compute(self, phase):
        """context of one compute section: its wall time (device synchronised on both sides) goes to stats[phase + "_s"]"""
        import contextlib

        @contextlib.contextmanager
        def section():
            lock = None
            if self.compute_lock:
                import fcntl
                lock = open(self.compute_lock, "a+")
                fcntl.flock(lock, fcntl.LOCK_EX)
            try:
                self.engine.sync()
                t0 = time.perf_counter()
                yield
                self.engine.sync()
                self.stats[phase + "_s"] += time.perf_counter() - t0
            finally:
                if lock is not None:
                    import fcntl
                    fcntl.flock(lock, fcntl.LOCK_UN)
                    lock.close()
        return section()

    def _phys(self, mask):
        return permute_mask(mask, self.perm)

    def _storage_real(self):
        return self.engine.tensor.dtype == torch.float64

    def _choose_storage(self, real_program):
        """before an initialisation: 8-byte amplitudes for a rotation list that keeps them real (engines that offer it)"""
        if hasattr(self.engine, "set_real"):
            want = bool(real_program and self.real_storage and self.n_local >= 2)
            if want != self._storage_real():
                self.engine.set_real(want, discard=True)
                self._tmp = None
                self._chunk_bufs = None

    def _complex_storage(self):
        if self._storage_real():
            self.engine.set_real(False)
            self._tmp = None
            self._chunk_bufs = None

    def _local_mask(self):
        return (1 << self.n_local) - 1

    def _tmp_buffer(self, count):
        if self._tmp is None or self._tmp.numel() < count or self._tmp.dtype != self.engine.tensor.dtype:
            self._tmp = None
            self._tmp = self.engine.new_buffer(count)
        return self._tmp[:count]

    #: pieces of one exchange: transfer k + 1 runs while piece k is unpacked into the shard / packed for sending
    EXCHANGE_PIECES = 8

    def _post_pair(self, snd, rcv, partner, tag=0):
        """post send + receive with ``partner`` -> object with ``wait()``.  RCCL takes the device tensors as they are.
        gloo (tests; CPU engines) does not synchronise with the GPU and talks to raw pointers, so device tensors travel
        through host copies there: sent from a host copy taken now, received into a host buffer that ``wait()`` copies
        to the device."""
        staged = snd.is_cuda and dist.get_backend(self.group) == "gloo"
        if snd.is_cuda and not staged and hasattr(self.engine, "check_stream"):
            self.engine.check_stream()
        s_buf = snd.cpu() if staged else snd
        r_buf = torch.empty(rcv.shape, dtype=rcv.dtype, device="cpu") if staged else rcv
        ops = [dist.P2POp(dist.isend, s_buf, partner, self.group, tag=tag), dist.P2POp(dist.irecv, r_buf, partner, self.group, tag=tag)]
        if self.rank > partner:   # lower rank sends first in a pair (gloo needs an order)
            ops.reverse()
        works = dist.batch_isend_irecv(ops)

        class _Pending:
            def wait(_self):
                for w in works:
                    w.wait()
                if staged:
                    rcv.copy_(r_buf)
                _self.keep = None

        pending = _Pending()
        pending.keep = (s_buf, r_buf)
        return pending

    def _exchange(self, partner, make_send, recv_pieces, on_arrival):
        """the piece pattern of an exchange with ONE partner and caller-made pieces (the transport check under RCCL,
        tests/test_gpu_nccl.py; ``_swap_bits`` posts its batches itself): piece p: ``make_send(p)`` then its send / receive is posted —
        RCCL orders each transfer behind the pack it depends on and runs the transfers in sequence on its own stream, so
        pack p + 1 and transfer p overlap; then every received piece is handed to ``on_arrival`` as soon as it has
        landed, while the later pieces are still on the link.  Lower rank sends first in a pair (gloo needs an order)."""
        works, keep = [], []
        for p, rcv in enumerate(recv_pieces):
            snd = make_send(p)
            keep.append(snd)
            if self.dry:     # (one rank alone: the piece it would send stands in for the piece it would receive)
                rcv.copy_(snd.view(rcv.shape))

                class _Done:
                    def wait(_self):
                        pass
                works.append(_Done())
                continue
            works.append(self._post_pair(snd, rcv, partner, tag=p))   # one tag per piece: gloo matches by tag
        for p, w in enumerate(works):
            w.wait()
            on_arrival(p)
            _progress()

    #: piece sets of an exchange in flight: while set p is on the links, set p + 1 is packed and set p - 1 unpacked
    EXCHANGE_DEPTH = 2

    def _scratch(self, count, real):
        """``count`` elements of exchange scratch: the shard's elements, or doubles for the real parts of a complex shard"""
        if real:
            return torch.view_as_real(self._tmp_buffer((count + 1) // 2)).reshape(-1)[:count]
        return self._tmp_buffer(count)

    def _block_index(self, mask, block, first, count):
        """shard positions of the amplitudes [first, first + count) of block ``block`` of the local bits ``mask`` (engines without
        pack / unpack: torch indexing)"""
        j = torch.arange(first, first + count, dtype=torch.int64, device=self.engine.tensor.device)
        fixed, i = 0, 0
        for bit in range(self.n_local):
            if (mask >> bit) & 1:
                j = ((j >> bit) << (bit + 1)) | (j & ((1 << bit) - 1))
                fixed |= ((block >> i) & 1) << bit
                i += 1
        return j | fixed

    def _pack(self, mask, block, first, count, dst, real):
        if hasattr(self.engine, "pack"):
            self.engine.pack(mask, block, first, count, dst, real)
        else:
            src = self.engine.tensor[self._block_index(mask, block, first, count)]
            dst.copy_(torch.view_as_real(src)[:, 0] if real else src)

    def _unpack(self, mask, block, first, count, src, real):
        if hasattr(self.engine, "unpack"):
            self.engine.unpack(mask, block, first, count, src, real)
        else:
            self.engine.tensor[self._block_index(mask, block, first, count)] = torch.complex(src, torch.zeros_like(src)) if real else src

    def _set_engine_tensor(self, tensor):
        if hasattr(self.engine, "set_tensor"):
            self.engine.set_tensor(tensor)
        else:
            self.engine.tensor = tensor

    def _swap_bits(self, gbits, lbits, also=None):
        """exchange the k physical global bits ``gbits`` with the k physical local bits ``lbits`` (pairwise) in one step: an all-to-all
        among the 2^k ranks of the sub-cube that ``gbits`` span.  The local bits split the shard into 2^k blocks; the rank with
        sub-cube coordinate a (its values on ``gbits``) keeps block a where it is and sends block b to the rank with coordinate b,
        where it lands as block a: S/2^k amplitudes to each of the 2^k - 1 partners, every partner over its own link, instead of S/2
        over one link k times.  A block travels in EXCHANGE_PIECES pieces; the pieces p of all partners are posted as one batch, and
        EXCHANGE_DEPTH batches are in flight: pack p + 1 and unpack p - 1 run while batch p is on the links.  Block b is received
        into scratch (its slot is the one being sent to b) and unpacked when its own piece has been packed: scratch is
        2 x EXCHANGE_DEPTH x (2^k - 1) pieces, (1 - 2^-k) S / 2 at the default sizes.  k = 1 is the half-shard exchange.
        ``also``: a second shard-sized buffer (lambda of the backward pass) that makes the same move right after the shard, as the
        engine's tensor for the duration of its run, through the same scratch: ONE exchange step — the permutation and
        stats["swaps"] advance once, the bytes count both vectors."""
        k = len(gbits)
        pairs = sorted(zip(lbits, gbits))               # block values count the local bits in ascending order
        lb, gb = [p[0] for p in pairs], [p[1] for p in pairs]
        if k < 1 or len(set(lb)) != k or len(set(gb)) != k or lb[-1] >= self.n_local or min(gb) < self.n_local or max(gb) >= self.n:
            raise ValueError("an exchange trades k distinct global bits for k distinct local bits")
        mask = sum(1 << b for b in lb)
        a = sum(((self.rank >> (gb[i] - self.n_local)) & 1) << i for i in range(k))
        gmask = sum(1 << (b - self.n_local) for b in gb)

        def rank_of(b):
            return (self.rank & ~gmask) | sum(((b >> i) & 1) << (gb[i] - self.n_local) for i in range(k))

        blocks = [b for b in range(1 << k) if b != a]
        bsize = 1 << (self.n_local - k)
        P = self.EXCHANGE_PIECES
        if k == 1:      # (the piece count of the half-shard exchange as it always was: rows of the strided half, or columns of few long rows)
            A, B = 1 << (self.n_local - 1 - lb[0]), 1 << lb[0]
            P = max(1, min(P, A)) if (A >= P or A >= B) else max(1, min(P, B))
        else:
            P = max(1, min(P, bsize))                   # never a zero-length piece: an empty send/recv pair is still a group launch
        cuts = [(bsize * p) // P for p in range(P + 1)]
        piece = max(cuts[p + 1] - cuts[p] for p in range(P))
        stored_real = self._storage_real()             # float64 shards travel as they are
        real = self.real and self.real_transfers and not stored_real     # (the same on every rank: the flag follows the rotation list)
        if also is not None and (real or stored_real):
            raise ValueError("a second vector travels with a complex shard only")
        # a block that is contiguous in the shard (the top local bits) is sent from where it lies
        in_place = mask == ((1 << k) - 1) << (self.n_local - k) and not real
        depth = max(1, min(self.EXCHANGE_DEPTH, P))
        nb = len(blocks)
        scratch = self._scratch(depth * nb * piece * (1 if in_place else 2), real)
        recv_sets = [[scratch[(s * nb + i) * piece:(s * nb + i + 1) * piece] for i in range(nb)] for s in range(depth)]
        send_sets = None if in_place else [[scratch[((depth + s) * nb + i) * piece:((depth + s) * nb + i + 1) * piece]
                                            for i in range(nb)] for s in range(depth)]
        self.engine.sync()
        _progress("half-shard exchange" if k == 1 else "%d-bit shard exchange" % k)
        t_swap = time.perf_counter()

        class _Done:
            def wait(_self):
                pass

        def post(p):
            first, count = cuts[p], cuts[p + 1] - cuts[p]
            s = p % depth
            items = []
            for i, b in enumerate(blocks):
                if in_place:
                    snd = self.engine.tensor[b * bsize + first:b * bsize + first + count]
                else:
                    snd = send_sets[s][i][:count]
                    self._pack(mask, b, first, count, snd, real)
                rcv = recv_sets[s][i][:count]
                if self.dry:     # (one rank alone: the piece it would send stands in for the piece it would receive)
                    rcv.copy_(snd)
                else:            # one tag per (piece, partner): gloo matches by tag, and both ends of a pair agree on it
                    items.append((snd, rcv, rank_of(b), (p << k) | (a ^ b)))
            return _Done() if self.dry else self._post_multi(items)

        def arrived(p, work):
            work.wait()
            first, count = cuts[p], cuts[p + 1] - cuts[p]
            for i, b in enumerate(blocks):
                self._unpack(mask, b, first, count, recv_sets[p % depth][i][:count], real)
            _progress()

        def move():
            pending = []
            for p in range(P):
                pending.append((p, post(p)))
                if len(pending) == depth:        # the buffers of this set are used again by piece p + 1
                    arrived(*pending.pop(0))
            while pending:
                arrived(*pending.pop(0))
            self.engine.sync()

        move()
        if also is not None:
            shard = self.engine.tensor
            self._set_engine_tensor(also)
            try:
                move()
            finally:
                self._set_engine_tensor(shard)
        self.stats["swap_s"] += time.perf_counter() - t_swap
        _progress("local sweeps")
        # the logical qubits living on each pair of physical bits trade places
        for lbit, gbit in pairs:
            la, lb_ = self.perm.index(gbit), self.perm.index(lbit)
            self.perm[la], self.perm[lb_] = lbit, gbit
        ebytes = 8 if (real or stored_real) else 16
        vectors = 1 if also is None else 2
        self.stats["swaps"] += 1
        self.stats["exchange_bits"] += k
        self.stats["bytes_sent"] += vectors * nb * bsize * ebytes
        self.stats["link_bytes"] += vectors * bsize * ebytes
        self.stats["real_exchanges"] += 1 if (real or stored_real) else 0
        self.stats["pieces"] += vectors * P

    @staticmethod
    def _use_lists(x_logical_seq, n):
        """per logical qubit: the (ascending) rotation numbers whose x mask touches it — next-use queries by bisection"""
        uses = [[] for _ in range(n)]
        for r, x in enumerate(x_logical_seq):
            m, b = int(x), 0
            while m:
                if m & 1:
                    uses[b].append(r)
                m >>= 1
                b += 1
        return uses

    def _localise(self, x_logical_seq, r, uses=None, swap=None):
        """make every X/Y qubit of rotation r local; victims by farthest next X/Y use (Belady).  ``uses``: _use_lists of the
        sequence (else scanned); ``swap``: what performs an exchange (default: the real one; the planner records instead)"""
        import bisect
        lmask = self._local_mask()
        swap = swap or self._swap_bits
        if self.max_exchange_bits > 1:
            return self._localise_multi(x_logical_seq, r, uses if uses is not None else self._use_lists(x_logical_seq, self.n), swap)
        while True:
            xp = self._phys(x_logical_seq[r])
            xg = xp & ~lmask
            if not xg:
                return xp
            gbit = xg.bit_length() - 1
            # candidate local physical bits not touched by this rotation's x
            best, best_next = None, -1
            for lbit in range(self.n_local - 1, -1, -1):
                if (xp >> lbit) & 1:
                    continue
                logical = self.perm.index(lbit)
                nxt = len(x_logical_seq) + 1
                if uses is not None:
                    u = uses[logical]
                    k = bisect.bisect_right(u, r)
                    if k < len(u):
                        nxt = u[k]
                else:
                    for s in range(r + 1, len(x_logical_seq)):
                        if (x_logical_seq[s] >> logical) & 1:
                            nxt = s
                            break
                if nxt > best_next:
                    best, best_next = lbit, nxt
            if best is None:
                raise ValueError("rotation touches more qubits than fit in one shard")
            swap([gbit], [best])

    def _localise_multi(self, x_logical_seq, r, uses, swap):
        """``_localise`` with exchanges of up to ``max_exchange_bits`` bits.  A k-bit exchange puts S/2^k on each of 2^k - 1 links
        where k half-shard exchanges put S/2 on one link k times, so the exchange that serves rotation r also brings in every global
        qubit that is needed sooner than a local qubit it can send away: the new global set is the g qubits outside r's x mask whose
        next X/Y use is farthest (never again = farthest; ties stay where they are — qubits global now first —, then the qubit on the
        highest physical bit: high local bits leave the longest contiguous runs to pack and unpack).  More
        moves than one exchange may trade: the qubits rotation r needs first, then those needed soonest, against the farthest local
        ones; the rest is planned again while r still has a global X/Y qubit.  Depends on the rotation list and the permutation
        only: the same plan on every rank."""
        import bisect
        lmask = self._local_mask()
        x, R = int(x_logical_seq[r]), len(x_logical_seq)

        def nxt(q):
            u = uses[q]
            i = bisect.bisect_right(u, r)
            return u[i] if i < len(u) else R + 1

        while True:
            xp = self._phys(x)
            if not xp & ~lmask:
                return xp
            cand = [q for q in range(self.n) if not (x >> q) & 1]
            if len(cand) < self.g:
                raise ValueError("rotation touches more qubits than fit in one shard")
            is_global = [self.perm[q] >= self.n_local for q in range(self.n)]
            cand.sort(key=lambda q: (-nxt(q), 0 if is_global[q] else 1, -self.perm[q]))
            keep = set(cand[:self.g])
            entering = [q for q in cand[:self.g] if not is_global[q]]                       # farthest next use first
            leaving = sorted((q for q in range(self.n) if is_global[q] and q not in keep),
                             key=lambda q: (0 if (x >> q) & 1 else 1, nxt(q), q))            # rotation r's own, then soonest
            m = min(len(leaving), self.max_exchange_bits)
            swap([self.perm[q] for q in leaving[:m]], [self.perm[q] for q in entering[:m]])

    # -- state ------------------------------------------------------------------------------
    def init_basis(self, logical_index):
        self.engine.init_basis(self._phys(logical_index))
        self.real = True

    def randomize(self, seed):
        """synthetic state defined on PHYSICAL indices (bench/scaling use; permutation reset)"""
        self.perm = list(range(self.n))
        self.real = False
        self._complex_storage()
        self.engine.randomize(seed, 1.0)
        n2 = torch.tensor([self.engine.norm2()], dtype=torch.float64, device=self.engine.tensor.device)
        if self._dist:
            dist.all_reduce(n2, group=self.group)
        self.engine.tensor.mul_(1.0 / float(n2.item()) ** 0.5)
        return float(n2.item())

    def norm2(self):
        n2 = torch.tensor([self.engine.norm2()], dtype=torch.float64, device=self.engine.tensor.device)
        if self._dist:
            dist.all_reduce(n2, group=self.group)
        return float(n2.item())

    # -- operations ---------------------------------------------------------------------------
    def apply_pauli_rotations(self, xs, zs, phis):
        """rotations in order, masks in LOGICAL index-bit space of the full register"""
        xs = [int(v) for v in xs]
        zs = [int(v) for v in zs]
        if self.real and any(not (bin(x & z).count("1") & 1) for x, z in zip(xs, zs)):
            self.real = False     # a string with an even number of Y (or a diagonal one) makes the amplitudes complex
        if not self.real:
            self._complex_storage()
        batch_x, batch_z, batch_p = [], [], []

        def flush():
            if batch_x:
                with self._compute("local_sweeps"):
                    self.engine.rotations(np.array(batch_x, np.uint64), np.array(batch_z, np.uint64),
                                          np.array(batch_p, np.float64))
                batch_x.clear(); batch_z.clear(); batch_p.clear()

        uses = self._use_lists(xs, self.n) if (len(xs) > 8 or self.max_exchange_bits > 1) else None
        for r in range(len(xs)):
            if self._phys(xs[r]) & ~self._local_mask():
                flush()  # the permutation is about to change: masks already queued used the old one
                xp = self._localise(xs, r, uses)
            else:
                xp = self._phys(xs[r])
            batch_x.append(xp)
            batch_z.append(self._phys(zs[r]))
            batch_p.append(float(phis[r]))
        flush()

    def apply_pauli_rotation(self, x, z, phi):
        self.apply_pauli_rotations([x], [z], [phi])

    def _group_by_partner(self, xs, zs, coeffs):
        """terms grouped by the GLOBAL part of their physical x mask (= the rank difference of the partner shard),
        in a rank-independent order"""
        groups = {}
        for t, (x, z, c) in enumerate(zip(xs, zs, coeffs)):
            xp, zp = self._phys(int(x)), self._phys(int(z))
            groups.setdefault(xp >> self.n_local, []).append((xp, zp, complex(c), t))
        return [(xg, groups[xg]) for xg in sorted(groups)]

    #: log2 of the amplitudes per chunk of a partner-shard read: at most 29 (8 GiB: the x bits of a term ABOVE the chunk cost extra
    #: passes of the cross-shard kernels — 34 qubits on 8 ranks: 44 / 41 / 37 / 32 passes per chunk set at 26 / 27 / 28 / 29 bits — so
    #: chunks are as large as the double buffers allow: 2 x 4 partners x 8 GiB beside a 32-GiB shard) and at least four chunks per
    #: shard (the transfer of chunk c + 1 hides behind the contraction of chunk c); OVQE_SHARD_CHUNK_BITS overrides it (tests)
    CHUNK_BITS = 29

    def _chunk_bits(self):
        import os
        env = os.environ.get("OVQE_SHARD_CHUNK_BITS")
        m = int(env) if env is not None else min(self.CHUNK_BITS, self.n_local - 2)
        return max(1, min(self.n_local, m))

    def _post_multi(self, items):
        """post every (send tensor or None, receive tensor or None, partner rank, tag) of ``items`` as ONE batch -> object with
        ``wait()``.  RCCL runs the transfers of a batch concurrently — one xGMI link per partner — and takes the device tensors as
        they are; gloo (tests; CPU engines) talks to raw host pointers, so device tensors travel through host copies there."""
        some = next(t for it in items for t in it[:2] if t is not None)
        staged = some.is_cuda and dist.get_backend(self.group) == "gloo"
        if some.is_cuda and not staged and hasattr(self.engine, "check_stream"):
            self.engine.check_stream()
        ops, keep = [], []
        sent = {}
        for snd, rcv, partner, tag in items:
            pair = []
            if snd is not None:
                if staged and id(snd) not in sent:
                    sent[id(snd)] = snd.cpu()          # (one host copy of the own chunk serves every destination)
                s_buf = sent[id(snd)] if staged else snd
                pair.append(dist.P2POp(dist.isend, s_buf, partner, self.group, tag=tag))
            if rcv is not None:
                r_buf = torch.empty(rcv.shape, dtype=rcv.dtype, device="cpu") if staged else rcv
                keep.append((r_buf, rcv))
                pair.append(dist.P2POp(dist.irecv, r_buf, partner, self.group, tag=tag))
            if len(pair) == 2 and self.rank > partner:   # lower rank sends first in a pair (gloo needs an order)
                pair.reverse()
            ops += pair
        works = dist.batch_isend_irecv(ops) if ops else []
        hold = list(sent.values())

        class _Pending:
            def wait(_self):
                for w in works:
                    w.wait()
                if staged:
                    for r_buf, rcv in keep:
                        rcv.copy_(r_buf)
                keep.clear()
                hold.clear()

        return _Pending()

    def _partner_chunks(self, partners, send_to=None, after_first_post=None):
        """generator over the chunks of the partners' psi shards: yields (c, [chunk c of the shard of rank ^ d for d in
        ``partners``]); this rank's own chunk c goes to rank ^ d for d in ``send_to`` (default: the same list — a symmetric read;
        the Hermitian halving of <H> reads from some partners and sends to others).  Chunk c + 1 of ALL partners is posted as one
        batch before chunk c is handed out (double buffering: 2 x len(partners) x 2^m amplitudes instead of two whole shards), so
        every link of the list carries traffic at once while the previous chunk is contracted ("several
        partners concurrently in chunks")."""
        send_to = list(partners) if send_to is None else list(send_to)
        partners = list(partners)
        if not partners and not send_to:
            return
        m = self._chunk_bits()
        csize = 1 << m
        nchunks = 1 << (self.n_local - m)
        np_ = len(partners)
        stored_real = self._storage_real()
        real = self.real and self.real_transfers and not stored_real
        if self.dry:     # one rank alone: its own chunks stand in for the partners' (same kernels, same bytes counted)
            if after_first_post is not None:
                after_first_post()
            for c in range(nchunks):
                own = self.engine.tensor[c * csize:(c + 1) * csize]
                self.stats["chunk_reads"] += np_
                self.stats["real_chunk_reads"] += np_ if (real or stored_real) else 0
                self.stats["bytes_sent"] += len(send_to) * csize * (8 if (real or stored_real) else 16)
                yield c, [own] * np_
                self.engine.sync()
            self.stats["full_shard_reads"] += np_
            self.stats["partners_per_read"] = max(self.stats["partners_per_read"], np_)
            return
        if np_ and (self._chunk_bufs is None or self._chunk_bufs[0].numel() < np_ * csize or self._chunk_bufs[0].dtype != self.engine.tensor.dtype):
            self._chunk_bufs = None
            self._chunk_bufs = [self.engine.new_buffer(np_ * csize), self.engine.new_buffer(np_ * csize)]
        self.engine.sync()

        if real and np_ and (self._chunk_real is None or self._chunk_real[0].numel() < np_ * csize):
            self._chunk_real = [torch.empty(np_ * csize, dtype=torch.float64, device=self.engine.tensor.device) for _ in range(2)]
        if real and send_to and (self._chunk_send is None or self._chunk_send[0].numel() != csize):   # (sized by the chunk alone: its own test)
            self._chunk_send = [torch.empty(csize, dtype=torch.float64, device=self.engine.tensor.device) for _ in range(2)]

        def post(c):
            # one tag per (chunk parity, partner difference): gloo matches by tag, and both ends of a pair agree on it
            own = self.engine.tensor[c * csize:(c + 1) * csize]
            if real and send_to:   # real parts only over the links; the complex chunks are rebuilt when the transfer has landed
                send = self._chunk_send[c & 1]
                send.copy_(torch.view_as_real(own)[:, 0])
                own = send
            into = self._chunk_real if real else self._chunk_bufs
            items = {}
            for d in send_to:
                items[d] = [own, None]
            for k, d in enumerate(partners):
                items.setdefault(d, [None, None])[1] = into[c & 1][k * csize:(k + 1) * csize]
            return self._post_multi([(sr[0], sr[1], self.rank ^ d, 2 * d + (c & 1)) for d, sr in sorted(items.items())])

        _progress("partner-shard read")
        pending = post(0)
        if after_first_post is not None:   # work that needs no partner data runs while the first chunks are on the links
            after_first_post()
        for c in range(nchunks):
            _progress()
            t0 = time.perf_counter()
            pending.wait()
            if hasattr(self.engine, "stream"):
                self.engine.stream.synchronize()      # the transfers themselves, for the link rates of the bench line
            self.stats["shard_read_s"] += time.perf_counter() - t0
            if real and np_:
                dst = torch.view_as_real(self._chunk_bufs[c & 1][:np_ * csize])
                dst[:, 0].copy_(self._chunk_real[c & 1][:np_ * csize])
                dst[:, 1].zero_()
            pending = post(c + 1) if c + 1 < nchunks else None
            self.stats["chunk_reads"] += np_
            self.stats["real_chunk_reads"] += np_ if (real or stored_real) else 0
            self.stats["bytes_sent"] += len(send_to) * csize * (8 if (real or stored_real) else 16)
            yield c, [self._chunk_bufs[c & 1][k * csize:(k + 1) * csize] for k in range(np_)]
            self.engine.sync()   # the buffers of this parity are posted again two chunks later
        self.stats["full_shard_reads"] += np_
        self.stats["partners_per_read"] = max(self.stats["partners_per_read"], np_)

    def _split_by_chunk(self, terms, xg):
        """terms of one partner group (physical masks) -> {h: (x_low, z_low, coefficient, z_high, x_high&z_high parity, t)} with
        h = the part of the local x mask ABOVE the chunk bits: the term pairs ket chunk c with bra chunk c ^ h"""
        m = self._chunk_bits()
        low = (1 << m) - 1
        lmask = self._local_mask()
        out = {}
        for xp, zp, c, t in terms:
            h = (xp & lmask) >> m
            ny_high = bin((xp & zp) >> m).count("1") & 3
            out.setdefault(h, []).append((xp & low, zp & low, c * (1j) ** ny_high, zp >> m, t))
        return out

    @staticmethod
    def _ket_sign(z_high, ket_high):
        return -1.0 if bin(z_high & ket_high).count("1") & 1 else 1.0

    def _remote_plan(self, groups):
        """[(xg, {h: terms})] for the partner groups + the list of rank differences, in a rank-independent order"""
        remote = [(xg, self._split_by_chunk(terms, xg)) for xg, terms in groups if xg]
        return remote, [xg for xg, _ in remote]

    # -- Hermitian sums: planned once per (term list, permutation) ----------------------------------------------------------------
    @staticmethod
    def share_of(rank, d, world, x_groups):
        """Which x-groups of the cross terms between ``rank`` and ``rank ^ d`` this RANK contracts.  A Hermitian term gives the pair
        (i on rank, j on rank ^ d) and its mirror image conjugate contributions, so ONE of the two ranks evaluates
        2 Re <shard|P|partner shard> and the other neither computes nor receives anything for it: half the contractions AND half the
        xGMI traffic of <H>.  The pairs are oriented like a round-robin tournament — rank r takes the partners s with
        1 <= (s - r) mod W < W/2: (W - 2)/2 each — and the diametric pair (d = W/2) shares its groups alternately.
        -> the sub-list of ``x_groups`` (sorted physical x masks)"""
        s = rank ^ d
        k = (s - rank) % world
        if 2 * k == world:
            return x_groups[0::2] if rank < s else x_groups[1::2]
        return list(x_groups) if 1 <= k < world / 2 else []

    def plan_hamiltonian(self, xs, zs, coeffs, constant=0.0):
        """plan of H = constant + sum_t c_t P_t (real c_t; logical masks) under the CURRENT permutation: the terms this rank
        evaluates for <H> — its d = 0 terms and, doubled, its share of the cross terms — as one engine sum; the partners it reads
        from / sends its shard to; the full list for sigma = H psi (planned at its first use)"""
        m = self._chunk_bits()
        phys = [(self._phys(int(x)), self._phys(int(z)), complex(c)) for x, z, c in zip(xs, zs, coeffs)]
        by_d = {}
        for xp, zp, c in phys:
            by_d.setdefault(xp >> self.n_local, {}).setdefault(xp, []).append((zp, c))
        ex, read_from, send_to = [], [], []
        for d in sorted(by_d):
            groups = sorted(by_d[d])
            if d == 0:
                ex += [(xp, zp, c) for xp in groups for zp, c in by_d[d][xp]]
                continue
            mine = self.share_of(self.rank, d, self.world, groups)
            ex += [(xp, zp, 2.0 * c) for xp in mine for zp, c in by_d[d][xp]]
            if mine:
                read_from.append(d)
            if self.share_of(self.rank ^ d, d, self.world, groups):
                send_to.append(d)
        # (the engine sums are made at their first use: an ADAPT screen never needs "expect", an energy never "apply")
        return {"m": m, "perm": tuple(self.perm), "const": float(np.real(constant)), "terms": phys, "expect_terms": ex,
                "read_from": read_from, "send_to": send_to, "partners": sorted(d for d in by_d if d), "expect": None, "apply": None}

    def _plan_sum(self, plan, which):
        if plan[which] is None:
            t = plan["expect_terms" if which == "expect" else "terms"]
            plan[which] = self.engine.plan_sum(np.array([v[0] for v in t], np.uint64), np.array([v[1] for v in t], np.uint64),
                                               np.array([v[2] for v in t], np.complex128), plan["m"])
        return plan[which]

    def free_plan(self, plan):
        for key in ("expect", "apply"):
            if plan.get(key) is not None:
                self.engine.free_sum(plan[key])
                plan[key] = None

    def _plan_for(self, xs, zs, coeffs, constant):
        """ad-hoc calls: the plans of the last few (term list, permutation) pairs are kept"""
        key = (tuple(self.perm), self._chunk_bits(), np.asarray(xs, np.uint64).tobytes(), np.asarray(zs, np.uint64).tobytes(),
               np.asarray(coeffs, np.complex128).tobytes())
        cache = self.__dict__.setdefault("_plans", {})
        plan = cache.pop(key, None)
        if plan is None:
            plan = self.plan_hamiltonian(xs, zs, coeffs, 0.0)
            while len(cache) >= 4:
                self.free_plan(cache.pop(next(iter(cache))))
        cache[key] = plan        # (most recently used last)
        plan["const"] = float(np.real(constant))
        return plan

    def expectation(self, xs, zs, coeffs, constant=0.0):
        """Re sum_t c_t <psi|P_t|psi> + constant over the whole register (same value on every rank)"""
        return self._expectation_planned(self._plan_for(xs, zs, coeffs, constant))

    def _expectation_planned(self, plan):
        if plan["perm"] != tuple(self.perm):
            raise ValueError("the Hamiltonian was planned under another qubit permutation")
        sid = self._plan_sum(plan, "expect")
        local = []

        def local_part():     # (posted first: the first chunk of every partner travels while the shard's own terms are evaluated)
            with self._compute("expectation_local"):
                local.append(self.engine.sum_expect_local(sid))

        for c, chunks in self._partner_chunks(plan["read_from"], plan["send_to"], after_first_post=local_part):
            with self._compute("expectation_remote"):
                for d, ket in zip(plan["read_from"], chunks):
                    self.engine.sum_expect_remote(sid, d, c, ket)
        if not local:
            local_part()      # (no partner at all: nothing was posted)
        total = local[0]
        if plan["read_from"]:
            total += self.engine.sum_expect_finish(sid).real
        val = torch.tensor([total], dtype=torch.float64, device=self.engine.tensor.device)
        _progress("all-reduce of the energy")
        if self._dist:
            dist.all_reduce(val, group=self.group)
        out = float(val.item()) + plan["const"]
        _progress("local sweeps")
        return out

    # -- ADAPT gradient screen on the sharded register ("ADAPT screen identical with sigma also sharded")
    def apply_hamiltonian(self, xs, zs, coeffs, constant=0.0, plan=None, keep_real=False):
        """sigma = (H + constant) psi, sharded like psi: the x_g = 0 terms act inside the shard; the other rank differences
        are accumulated chunk by chunk from the partners' psi shards (all partners of a chunk in flight at once).
        ``keep_real``: a float64 shard stays float64 and sigma is a float64 buffer (the caller has checked that H maps real
        vectors to real vectors: the planned ADAPT screen); otherwise the shard is widened to complex amplitudes first.
        -> this rank's sigma shard (device buffer owned by the caller until the next call)"""
        size = 1 << self.n_local
        if not (keep_real and self._storage_real()):
            self._complex_storage()   # (sigma = H psi and what is built on it work on complex amplitudes)
        if getattr(self, "_sigma", None) is None or self._sigma.numel() < size or self._sigma.dtype != self.engine.tensor.dtype:
            self._sigma = None
            self._sigma = self.engine.new_buffer(size)
        sigma = self._sigma[:size]
        plan = plan if plan is not None else self._plan_for(xs, zs, coeffs, constant)
        if plan["perm"] != tuple(self.perm):
            raise ValueError("the Hamiltonian was planned under another qubit permutation")
        return self._apply_planned(plan, sigma, float(np.real(constant)))

    def _apply_planned(self, plan, sigma, ident):
        """sigma <- (H + ident) psi with the planned "apply" sum, psi = the engine's state buffer in its current storage (on float64
        shards the partner chunks travel as doubles and the engine contracts them as such)"""
        sid = self._plan_sum(plan, "apply")
        with self._compute("apply"):
            self.engine.sum_apply_local(sid, sigma, ident)
        for c, chunks in self._partner_chunks(plan["partners"]):
            with self._compute("apply"):
                for d, ket in zip(plan["partners"], chunks):
                    self.engine.sum_apply_remote(sid, d, c, ket, sigma)
        self.engine.sync()
        return sigma

    # -- lowest eigenpair of a Hermitian Pauli sum: Lanczos over the shards ---------------------------------------------------------
    def _all_sum(self, *values):
        """the sums over the ranks of a few local scalars (one all-reduce)"""
        buf = torch.tensor([float(v) for v in values], dtype=torch.float64, device=self.engine.tensor.device)
        if self._dist:
            dist.all_reduce(buf, group=self.group)
        return [float(v) for v in buf.cpu()]

    def _vec_dot(self, a, b):
        if hasattr(self.engine, "vec_dot"):
            return complex(self.engine.vec_dot(a, b))
        return complex(torch.vdot(a, b).item())

    def _vec_update(self, w, v, vprev, alpha, beta):
        if hasattr(self.engine, "vec_update"):
            return float(self.engine.vec_update(w, v, vprev, alpha, beta))
        w.add_(v, alpha=-alpha)
        if vprev is not None:
            w.add_(vprev, alpha=-beta)
        return float(torch.vdot(w, w).real.item())

    def _vec_scale(self, v, s):
        if hasattr(self.engine, "vec_scale"):
            self.engine.vec_scale(v, s)
        else:
            v.mul_(s)

    def _vec_axpy(self, y, x, s, overwrite=False):
        if hasattr(self.engine, "vec_axpy"):
            self.engine.vec_axpy(y, x, s, overwrite)
        elif overwrite:
            torch.mul(x, s, out=y)
        else:
            y.add_(x, alpha=s)

    def ground_state(self, xs, zs, coeffs, constant=0.0, tol=1e-10, max_iter=3000, seed=20250227):
        """Lowest eigenpair of H = constant + sum_t c_t P_t (real c_t, logical masks) by Lanczos on the partitioned register
        -> (energy, residual |H y - E y|, steps), the same numbers on every rank; ``tol``, ``max_iter`` and ``seed`` mean what they
        mean to ``backend.Statevector.ground_state``.  Afterwards the register holds the normalised eigenvector y under the
        identity permutation.

        Two passes of the three-term recurrence: the algorithm of ``lanczos_lowest`` (csrc/sv_lanczos_host.hpp), which the
        one-device solvers run, restated here over the shards.  Pass 1 builds the tridiagonal matrix (stop test
        |beta_m s_m| < tol max(1, |lambda|) every fifth step), pass 2 repeats it from the same seeded start and accumulates the Ritz vector; then the Rayleigh quotient and the true residual of y.  NO Lanczos vector is
        kept at shard size — at the register sizes this path is for nothing is left to keep them in: a rank holds four
        shard-sized vectors (v_{j-1}, v_j, w and y) and the double buffers of the partner chunks, whatever the step count.
        alpha_j and beta_j are all-reduced before any use (two all-reduces per step), so every rank solves the identical
        tridiagonal matrix on the host and stops at the same step.

        Storage: float64 shards when every string has an even number of Y (a real-symmetric H: every Jordan-Wigner molecular
        Hamiltonian; its Krylov vectors stay real) and the engine offers ``set_real`` — half the HBM bytes per vector and per
        sigma = H psi pass and half the link bytes per partner chunk; complex128 otherwise."""
        from scipy.linalg import eigh_tridiagonal
        cs = np.asarray(coeffs, np.complex128).reshape(-1)
        if np.any(cs.imag != 0.0):
            raise ValueError("ground_state: a Hermitian sum has real coefficients")
        if not hasattr(self.engine, "randomize"):
            raise NotImplementedError("this shard engine has no randomize (the seeded start vector)")
        xs = [int(v) for v in xs]
        zs = [int(v) for v in zs]
        size = 1 << self.n_local
        self.perm = list(range(self.n))
        real = bool(all(not (bin(x & z).count("1") & 1) for x, z in zip(xs, zs)) and hasattr(self.engine, "set_real")
                    and self.real_storage and self.n_local >= 2)
        if hasattr(self.engine, "set_real"):
            self.engine.set_real(real, discard=True)
        self._tmp = self._chunk_bufs = self._sigma = None
        self.real = real          # (the partner chunks of a complex Krylov vector travel whole)
        plan = self._plan_for(xs, zs, cs.real, 0.0)
        bufs = [self.engine.tensor] + [self.engine.new_buffer(size) for _ in range(3)]
        y = bufs[3]
        max_iter = int(min(max(int(max_iter), 1), 1 << self.n))
        alpha, beta = [], []
        state = {"m": 0, "lam": 0.0, "s": None}

        def lowest():
            m = state["m"]
            if m == 1:
                return alpha[0], np.ones(1)
            w, v = eigh_tridiagonal(np.array(alpha[:m]), np.array(beta[:m - 1]), select="i", select_range=(0, 0))
            return float(w[0]), v[:, 0]

        def start(B):
            self._set_engine_tensor(B)
            self.engine.randomize(seed, 1.0)
            n2, = self._all_sum(self.engine.norm2())
            self._vec_scale(B, 1.0 / n2 ** 0.5)

        def recurrence(accumulate):
            A, B, C = bufs[0], bufs[1], bufs[2]
            start(B)
            s = state["s"]
            if accumulate:
                self._vec_axpy(y, B, float(s[0]), overwrite=True)
            steps = state["m"] - 1 if accumulate else max_iter
            for j in range(steps):
                _progress("Lanczos")
                self._set_engine_tensor(B)
                self._apply_planned(plan, C, 0.0)
                if accumulate:
                    self._vec_update(C, B, A if j else None, alpha[j], beta[j - 1] if j else 0.0)
                    bj = beta[j]
                else:
                    a, = self._all_sum(self._vec_dot(B, C).real)
                    alpha.append(a)
                    b2, = self._all_sum(self._vec_update(C, B, A if j else None, a, beta[j - 1] if j else 0.0))
                    bj = max(b2, 0.0) ** 0.5
                    state["m"] = j + 1
                    last = j + 1 == steps or bj < 1e-13 * max(1.0, abs(a))
                    if last or (j >= 4 and j % 5 == 4):
                        state["lam"], state["s"] = lowest()
                        est = abs(bj * state["s"][-1])
                        if last or est < tol * max(1.0, abs(state["lam"])):
                            return
                    beta.append(bj)
                self._vec_scale(C, 1.0 / bj)
                A, B, C = B, C, A
                if accumulate:
                    self._vec_axpy(y, B, float(s[j + 1]))

        recurrence(False)     # pass 1: the tridiagonal matrix
        recurrence(True)      # pass 2: the Ritz vector, same recurrence
        _progress("Lanczos")
        self._set_engine_tensor(y)
        n2, = self._all_sum(self._vec_dot(y, y).real)
        self._vec_scale(y, 1.0 / n2 ** 0.5)
        sigma = bufs[0]
        self._apply_planned(plan, sigma, 0.0)
        lam, = self._all_sum(self._vec_dot(y, sigma).real)
        r2, = self._all_sum(self._vec_update(sigma, y, None, lam, 0.0))
        self.engine.sync()
        _progress("local sweeps")
        return lam + float(np.real(constant)), max(r2, 0.0) ** 0.5, state["m"]

    #: planned pools kept (most recently used last); the evicted ones are freed
    POOL_PLANS_KEPT = 4

    def _pool_plan_for(self, pool):
        """the engine plan of ``pool`` under the CURRENT permutation and chunk size, made once: key = (permutation, chunk bits, the
        pool's terms)"""
        counts = np.array([len(op[0]) for op in pool], np.int64)
        offsets = np.zeros(len(pool) + 1, np.int64)
        np.cumsum(counts, out=offsets[1:])
        xs = np.array([int(x) for op in pool for x in op[0]], np.uint64)
        zs = np.array([int(z) for op in pool for z in op[1]], np.uint64)
        cs = np.array([complex(c) for op in pool for c in op[2]], np.complex128)
        m = self._chunk_bits()
        key = (tuple(self.perm), m, offsets.tobytes(), xs.tobytes(), zs.tobytes(), cs.tobytes())
        cache = self.__dict__.setdefault("_pool_plans", {})
        plan = cache.pop(key, None)
        if plan is None:
            px = np.array([self._phys(int(x)) for x in xs], np.uint64)
            pz = np.array([self._phys(int(z)) for z in zs], np.uint64)
            pid = self.engine.plan_pool(offsets, px, pz, cs, m)
            self.stats["pool_plans"] += 1
            plan = {"pid": pid, "partners": [d for d, _ in self.engine.pool_partners(pid)], "n_ops": len(pool)}
            while len(cache) >= self.POOL_PLANS_KEPT:
                self.engine.free_pool(cache.pop(next(iter(cache)))["pid"])
        cache[key] = plan
        return plan

    def free_pool_plans(self):
        cache = self.__dict__.get("_pool_plans") or {}
        while cache:
            self.engine.free_pool(cache.pop(next(iter(cache)))["pid"])

    def pool_gradients(self, ham, pool, mode="fermionic"):
        """ADAPT screen over ``pool`` = [(xs, zs, coeffs) per operator] with H = (ham_xs, ham_zs, ham_coeffs, constant):
        sigma = H psi once (sharded), then v_k = sum_j c_j <sigma|P_j|psi>; g_k = 2 Re v_k (fermionic,
        ref:openvqe/adapt/fermionic_adapt_vqe.py:67-73) or 2 |v_k| (qubit, ref:openvqe/adapt/qubit_adapt_vqe.py:147-150).  Same
        values on every rank.

        Engines that offer ``plan_pool`` (the HIP engine): the pool is planned once per (permutation, chunk bits, pool) and a screen
        is one ``pool_local`` — while the first chunks travel —, one ``pool_remote`` per (partner, chunk), one ``pool_finish`` and one
        all-reduce of the n_ops complex values; its seconds go to stats["screen_s"].  A float64 shard whose state is real stays
        float64 when H maps real vectors to real vectors (every string an even number of Y, real coefficients): sigma, the chunks on
        the links and the screen are then doubles.  Other engines: one batched contraction per (rank difference, chunk pair),
        re-planned at every call."""
        if not hasattr(self.engine, "plan_pool"):
            return self._pool_gradients_unplanned(ham, pool, mode)
        hx, hz, hc, const = ham
        hcs = np.asarray(hc, np.complex128).reshape(-1)
        keep_real = bool(self._storage_real() and self.real and np.all(hcs.imag == 0.0) and complex(const).imag == 0.0 and
                         all(not (bin(int(x) & int(z)).count("1") & 1) for x, z in zip(hx, hz)))
        sigma = self.apply_hamiltonian(hx, hz, hc, const, keep_real=keep_real)
        plan = self._pool_plan_for(pool)
        pid, partners = plan["pid"], plan["partners"]
        done = []

        def local_part():     # (posted first: the first chunk of every partner travels while the shard's own entries are contracted)
            with self._compute("screen"):
                self.engine.pool_local(pid, sigma)
            done.append(True)

        for c, chunks in self._partner_chunks(partners, after_first_post=local_part):
            with self._compute("screen"):
                for d, ket in zip(partners, chunks):
                    self.engine.pool_remote(pid, d, c, ket, sigma)
        if not done:
            local_part()      # (no partner at all: nothing was posted)
        with self._compute("screen"):
            vals = np.asarray(self.engine.pool_finish(pid), np.complex128)
        buf = torch.from_numpy(np.stack([vals.real, vals.imag])).to(self.engine.tensor.device)
        _progress("all-reduce of the pool gradients")
        if self._dist:
            dist.all_reduce(buf, group=self.group)
        v = buf[0].cpu().numpy() + 1j * buf[1].cpu().numpy()
        _progress("local sweeps")
        return 2.0 * v.real if mode == "fermionic" else 2.0 * np.abs(v)

    def _pool_gradients_unplanned(self, ham, pool, mode="fermionic"):
        """(engines without ``plan_pool``) ADAPT screen over ``pool`` = [(xs, zs, coeffs) per operator] with H = (ham_xs, ham_zs, ham_coeffs, constant):
        sigma = H psi once (sharded), then v_k = sum_j c_j <sigma|P_j|psi> with the pool terms grouped by partner shard
        — one batched launch per (rank difference, chunk pair) —, one all-reduce of the n_ops complex values;
        g_k = 2 Re v_k (fermionic, ref:openvqe/adapt/fermionic_adapt_vqe.py:67-73) or 2 |v_k| (qubit,
        ref:openvqe/adapt/qubit_adapt_vqe.py:147-150).  Same values on every rank."""
        hx, hz, hc, const = ham
        sigma = self.apply_hamiltonian(hx, hz, hc, const)
        flat = [(int(x), int(z), complex(c), k) for k, (xs, zs, cs) in enumerate(pool) for x, z, c in zip(xs, zs, cs)]
        groups = self._group_by_partner([f[0] for f in flat], [f[1] for f in flat], [f[2] for f in flat])
        owner = [f[3] for f in flat]
        vals = np.zeros(len(pool), np.complex128)

        def csr(terms, coeff_of):
            # CSR over the operators that have terms in this group (operator order kept)
            by_op = {}
            for t in terms:
                by_op.setdefault(owner[t[-1]], []).append(t)
            ops = sorted(by_op)
            offsets = np.zeros(len(ops) + 1, np.int64)
            xs, zs, cs = [], [], []
            for i, k in enumerate(ops):
                offsets[i + 1] = offsets[i] + len(by_op[k])
                for t in by_op[k]:
                    xs.append(t[0]); zs.append(t[1]); cs.append(coeff_of(t))
            return ops, offsets, np.array(xs, np.uint64), np.array(zs, np.uint64), np.array(cs, np.complex128)

        for xg, terms in groups:
            if xg == 0:
                ops, offsets, txs, tzs, tcs = csr(terms, lambda t: t[2])
                vals[ops] += self.engine.bilinear_batch(offsets, txs, tzs, tcs, sigma, None)
        remote, partners = self._remote_plan(groups)
        m = self._chunk_bits()
        for c, chunks in self._partner_chunks(partners):
            for (xg, by_h), ket in zip(remote, chunks):
                ket_high = ((self.rank ^ xg) << (self.n_local - m)) | c
                for h, terms in sorted(by_h.items()):
                    ops, offsets, txs, tzs, tcs = csr(terms, lambda t: t[2] * self._ket_sign(t[3], ket_high))
                    vals[ops] += self.engine.sub_bilinear_batch(m, offsets, txs, tzs, tcs, sigma, (c ^ h) << m, ket)
        buf = torch.from_numpy(np.stack([vals.real, vals.imag])).to(self.engine.tensor.device)
        if self._dist:
            dist.all_reduce(buf, group=self.group)
        v = buf[0].cpu().numpy() + 1j * buf[1].cpu().numpy()
        return 2.0 * v.real if mode == "fermionic" else 2.0 * np.abs(v)

    # -- compiled programs: the exchange plan of a rotation list is made ONCE (ref:openvqe/ucc_family/get_energy_ucc.py:42-45 runs the
    # same list with new angles at every optimiser step) -----------------------------------------------------------------------
    def compile_program(self, rot_xs, rot_zs, rot_coeffs, rot_pidx, hf_index, hamiltonian=None, rot_phi0=None):
        """plan of `|hf> -> prod_r exp(-i coeff_r theta[pidx_r] P_r)` on this partition, from the identity permutation: the
        half-shard exchanges (Belady victims over the whole list, next uses by bisection: O(R n log R) instead of the O(R^2 n) scan)
        and, between them, the local rotations with their masks already in PHYSICAL bit space; with ``hamiltonian`` =
        (xs, zs, coeffs, constant) also its terms grouped by partner shard under the program's FINAL permutation.
        -> an object for ``run_program`` / ``program_energy``; identical on every rank"""
        xs = [int(v) for v in rot_xs]
        zs = [int(v) for v in rot_zs]
        saved = list(self.perm)
        self.perm = list(range(self.n))
        uses = self._use_lists(xs, self.n)
        steps, batch = [], []

        def record_swap(gbits, lbits):
            for gbit, lbit in zip(gbits, lbits):
                la, lb = self.perm.index(gbit), self.perm.index(lbit)
                self.perm[la], self.perm[lb] = lbit, gbit
            steps.append(("swap", tuple(gbits), tuple(lbits)))

        def flush():
            if batch:
                idx = np.array([b[0] for b in batch], np.int64)
                steps.append(("rot", np.array([b[1] for b in batch], np.uint64), np.array([b[2] for b in batch], np.uint64), idx))
                batch.clear()

        try:
            for r in range(len(xs)):
                if self._phys(xs[r]) & ~self._local_mask():
                    flush()
                    xp = self._localise(xs, r, uses, swap=record_swap)
                else:
                    xp = self._phys(xs[r])
                batch.append((r, xp, self._phys(zs[r])))
            flush()
            final_perm = list(self.perm)
            prog = {"steps": steps, "coeff": np.asarray(rot_coeffs, np.float64), "pidx": np.asarray(rot_pidx, np.int64),
                    "phi0": None if rot_phi0 is None else np.asarray(rot_phi0, np.float64),
                    "hf": int(hf_index), "perm": final_perm, "real": all(bin(x & z).count("1") & 1 for x, z in zip(xs, zs)),
                    "swaps": sum(1 for st in steps if st[0] == "swap"), "ham": None,
                    # bits per exchange, in order: exchange e puts S / 2^k_e on its busiest link and sends (1 - 2^-k_e) S in all
                    "exchange_bits": [len(st[1]) for st in steps if st[0] == "swap"],
                    "n_params": int(np.asarray(rot_pidx, np.int64).max(initial=-1)) + 1}
            if hamiltonian is not None:
                hx, hz, hc, const = hamiltonian
                prog["ham"] = self.plan_hamiltonian(hx, hz, hc, const)   # under the final permutation (self.perm right now)
        finally:
            self.perm = saved
        return prog

    @staticmethod
    def _program_angles(prog, theta):
        """rotation r: exp(-i (coeff_r theta[pidx_r] + phi0_r) P_r); pidx_r < 0: a constant angle — phi0_r when the program carries
        constants (ovqe_set_program's convention), else coeff_r"""
        pidx = prog["pidx"]
        fixed = 1.0 if prog.get("phi0") is None else 0.0
        phis = prog["coeff"] * (np.where(pidx >= 0, theta[np.maximum(pidx, 0)], fixed) if theta.size else fixed)
        if prog.get("phi0") is not None:
            phis = phis + prog["phi0"]
        return phis

    def run_program(self, prog, theta):
        """|hf> -> the program's state at ``theta`` (the plan's exchanges and local sweeps; no planning)"""
        theta = np.asarray(theta, np.float64).reshape(-1)
        if theta.size < prog["n_params"]:
            raise ValueError(f"expected {prog['n_params']} parameters, got {theta.size}")
        self.perm = list(range(self.n))
        self._choose_storage(prog["real"])
        self.init_basis(prog["hf"])
        self.real = prog["real"]      # (a list with one even-Y string anywhere travels complex from the start: the flag is per program)
        phis = self._program_angles(prog, theta)
        for st in prog["steps"]:
            if st[0] == "swap":
                self._swap_bits(st[1], st[2])
            else:
                with self._compute("local_sweeps"):
                    self.engine.rotations(st[1], st[2], phis[st[3]])
        assert self.perm == prog["perm"]

    def program_energy(self, prog, theta):
        """E(theta) = <psi(theta)|H|psi(theta)> + constant with the Hamiltonian the program was compiled with"""
        if prog["ham"] is None:
            raise ValueError("compile_program was called without a Hamiltonian")
        self.run_program(prog, theta)
        return self._expectation_planned(prog["ham"])

    def program_energy_gradient(self, prog, theta):
        """E(theta) and dE/dtheta[K] by the adjoint method on the shards (same values on every rank): the forward plan, lambda = H psi
        with the program's Hamiltonian plan (E = Re <psi|lambda> + constant comes from it: nothing is planned or contracted twice),
        then the plan's steps in REVERSE on psi and lambda together — a rotation step gives this shard's sums
        w_r = Im <lambda|P_r|psi> and un-rotates both vectors (``engine.adjoint_rotations``), an exchange step is replayed for both
        (disjoint bit swaps are their own inverse) —, ONE all-reduce of the R sums and the energy;
        dE/dtheta_p = sum_{r: pidx_r = p} 2 coeff_r w_r (constant-angle rotations are un-rotated and contribute nothing).
        A real program runs forward on float64 shards and is widened once, before lambda.  The backward pass works in place on the
        shard and on the sigma buffer of ``apply_hamiltonian``: no further shard-sized allocation.
        AFTER the call the register holds |hf> (complex storage, identity permutation) and the sigma buffer U^+ H psi — NOT
        psi(theta); ``run_program`` prepares it again."""
        if prog["ham"] is None:
            raise ValueError("compile_program was called without a Hamiltonian")
        if not hasattr(self.engine, "adjoint_rotations"):
            raise NotImplementedError("this shard engine has no adjoint_rotations")
        theta = np.asarray(theta, np.float64).reshape(-1)
        self.run_program(prog, theta)
        phis = self._program_angles(prog, theta)
        plan = prog["ham"]
        self._complex_storage()
        lam = self.apply_hamiltonian(None, None, None, 0.0, plan=plan)   # (partner reads of a real psi still move real parts only)
        self.real = False             # lambda = H psi is complex in general: from here both vectors travel as complex amplitudes
        one = self.engine.bilinear_batch(np.array([0, 1], np.int64), np.zeros(1, np.uint64), np.zeros(1, np.uint64),
                                         np.ones(1, np.complex128), lam, None)      # <lambda|psi> over this shard
        w = np.zeros(len(prog["coeff"]) + 1, np.float64)
        w[-1] = float(np.real(np.asarray(one).reshape(-1)[0]))
        for st in reversed(prog["steps"]):
            if st[0] == "swap":
                self._swap_bits(st[1], st[2], also=lam)
            else:
                _progress("adjoint sweeps")
                with self._compute("adjoint_sweeps"):
                    w[st[3]] = self.engine.adjoint_rotations(lam, st[1], st[2], phis[st[3]])
        assert self.perm == list(range(self.n))
        buf = torch.from_numpy(w).to(self.engine.tensor.device)
        _progress("all-reduce of the gradient")
        if self._dist:
            dist.all_reduce(buf, group=self.group)
        w = buf.cpu().numpy()
        _progress("local sweeps")
        pidx = prog["pidx"]
        grad = np.zeros(prog["n_params"], np.float64)
        live = pidx >= 0
        np.add.at(grad, pidx[live], 2.0 * prog["coeff"][live] * w[:-1][live])
        return float(w[-1]) + plan["const"], grad

    def energy(self, ham_xs, ham_zs, ham_coeffs, constant, rot_xs, rot_zs, rot_phis, hf_index):
        """one whole evaluation: |hf> -> rotations -> <H>"""
        self.perm = list(range(self.n))
        self._choose_storage(all(bin(int(x) & int(z)).count("1") & 1 for x, z in zip(rot_xs, rot_zs)) and len(rot_xs) > 0)
        self.init_basis(hf_index)
        self.apply_pauli_rotations(rot_xs, rot_zs, rot_phis)
        return self.expectation(ham_xs, ham_zs, ham_coeffs, constant)

    # -- read-back (tests / small registers) ------------------------------------------------------
    def gather_state(self):
        """full state in LOGICAL index order on every rank (small n only)"""
        if self._storage_real():
            self._complex_storage()
        shard = self.engine.tensor.detach().to("cpu")
        if self.world > 1:
            parts = [torch.empty_like(shard) for _ in range(self.world)]
            if self.engine.tensor.is_cuda:
                dev_parts = [torch.empty_like(self.engine.tensor) for _ in range(self.world)]
                dist.all_gather(dev_parts, self.engine.tensor, group=self.group)
                parts = [p.cpu() for p in dev_parts]
            else:
                dist.all_gather(parts, shard, group=self.group)
            phys = torch.cat(parts).numpy()
        else:
            phys = shard.numpy()
        idx = np.arange(1 << self.n, dtype=np.int64)
        pidx = np.zeros_like(idx)
        for b in range(self.n):
            pidx |= ((idx >> b) & 1) << self.perm[b]
        return phys[pidx]
