"""The exact (adjoint-method) gradient on the index-bit-partitioned register: ``ShardedStatevector.program_energy_gradient`` —
forward plan, lambda = H psi, the plan's steps in reverse on psi and lambda together, one all-reduce — and its public face
``PartitionedStatevector.energy_gradient`` behind ``UCCEvaluator.energy_gradient`` / ``EnergyUCC.adjoint_gradient``
(ref:openvqe/ucc_family/get_energy_ucc.py:42-50,158-175).  Shard arithmetic by the oracle engine of tests/test_distributed.py
(plus the backward step, below) over gloo; the checker is ``oracle.masks.ucc_energy_gradient`` on the whole register.
The same workers run on HIP shards in tests/test_gpu_shard_gradient.py.

Bound: |dE| and max |d grad| < 1e-11 * ||H||_1, what tests/test_gpu_sector.py holds the one-device gradient paths to."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import masks
from tests.oracle_backend import OracleStatevector
from tests.test_distributed import OracleShardEngine, _free_port

BOUND = 1e-11      # times ||H||_1


class AdjointOracleEngine(OracleShardEngine):
    """the CPU shard engine with the backward step of the adjoint method (the engine protocol's ``adjoint_rotations``)"""

    def adjoint_rotations(self, lam, xs, zs, phis):
        psi, l = self._np(), lam.numpy()
        w = np.zeros(len(xs))
        for r in range(len(xs) - 1, -1, -1):
            x, z, p = int(xs[r]), int(zs[r]), float(phis[r])
            assert x >> self.n_local == 0
            w[r] = np.vdot(l, masks.pauli_apply(psi, x, z, index_offset=self.base)).imag
            psi[:] = np.cos(p) * psi + 1j * np.sin(p) * masks.pauli_apply(psi, x, z, index_offset=self.base)
            l[:] = np.cos(p) * l + 1j * np.sin(p) * masks.pauli_apply(l, x, z, index_offset=self.base)
        return w


class AnalyticOracleStatevector(OracleStatevector):
    """the single-process stand-in with the ANALYTIC gradient of the oracle (the base class differentiates numerically)"""

    def energy_gradient(self, theta):
        _, xs, zs, cs, p0, pi, hf = self._prog
        hx, hz, hc, const = self._ham
        theta = np.asarray(theta, float).reshape(-1)[: self._K]
        return masks.ucc_energy_gradient(self.nbqbits, hf, xs, zs, cs, pi, theta, hx, hz, hc, const, phi0=p0)


def draw_case(rng, n, g, even):
    """a rotation list as in tests/test_distributed.py (36 rotations of weight 2-4, x masks anywhere: on the rank bits too) and a real
    symmetric Hamiltonian.  even = False: every string has one Y (a real program), shared parameters, some constant-angle
    rotations (pidx < 0) and a phi0;  even = True: strings with two Y and diagonal rotations — complex from the start."""
    K, R, T = 7, 36, 30
    xs, zs = [], []
    for _ in range(R):
        w = int(rng.integers(2, max(3, min(5, n - g))))
        bits = [int(b) for b in rng.choice(n, w, replace=False)]
        x = sum(1 << b for b in bits)
        z = 1 << bits[0]
        if even:
            z |= 1 << bits[1]
        for b in rng.choice(n, 2, replace=False):
            if not (x >> int(b)) & 1:
                z |= 1 << int(b)
        if even and rng.random() < 0.2:
            x = 0
        xs.append(x); zs.append(z)
    coeff = rng.uniform(0.5, 1.5, R)
    pidx = rng.integers(0, K, R)
    phi0 = None
    if not even:
        pidx[rng.choice(R, 5, replace=False)] = -1
        phi0 = rng.uniform(-0.4, 0.4, R)
    hx = [sum(1 << int(b) for b in rng.choice(n, int(rng.integers(1, 4)), replace=False)) if rng.random() < 0.85 else 0 for _ in range(T)]
    hz = []
    for x in hx:      # an even number of Y per term: a real symmetric H
        z = int(rng.integers(0, 1 << n))
        if bin(x & z).count("1") & 1:
            z ^= x & -x
        hz.append(z)
    hc = rng.normal(size=T)
    hf = int(rng.integers(0, 1 << n))
    theta = rng.uniform(-0.8, 0.8, K)
    return dict(xs=xs, zs=zs, coeff=coeff, pidx=pidx, phi0=phi0, hx=hx, hz=hz, hc=hc, const=0.75, hf=hf, theta=theta)


def same_x_chunks(prog, cap=16):
    """backward passes of the streaming kernels over the program: one per same-x run of a rotation step, in chunks of ``cap``"""
    total = 0
    for st in prog["steps"]:
        if st[0] != "rot":
            continue
        xs = [int(v) for v in st[1]]
        a = 0
        while a < len(xs):
            b = a + 1
            while b < len(xs) and xs[b] == xs[a]:
                b += 1
            total += -(-(b - a) // cap)
            a = b
    return total


def gradient_worker(rank, world, port, n, seed, out, engine="oracle", chunk_bits=3):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["OVQE_SHARD_CHUNK_BITS"] = str(chunk_bits)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from openvqe_amd.distributed import ShardedStatevector
        rng = np.random.default_rng(seed)
        g = world.bit_length() - 1
        res = []
        for even in (False, True):
            case = draw_case(rng, n, g, even)
            sv = (ShardedStatevector(n, device=0) if engine == "hip" else
                  ShardedStatevector(n, engine_factory=lambda nl, ng, r: AdjointOracleEngine(nl, ng, r)))
            prog = sv.compile_program(case["xs"], case["zs"], case["coeff"], case["pidx"], case["hf"],
                                      hamiltonian=(case["hx"], case["hz"], case["hc"], case["const"]), rot_phi0=case["phi0"])
            th = case["theta"]

            def delta(fn):
                before = dict(sv.stats)
                fn()
                return {k: sv.stats[k] - before[k] for k in ("swaps", "bytes_sent")}

            def forward_and_lambda():
                sv.run_program(prog, th)
                sv._complex_storage()
                sv.apply_hamiltonian(None, None, None, 0.0, plan=prog["ham"])

            d_fwd = delta(forward_and_lambda)                  # what the gradient does before its backward pass
            sv.real_storage = sv.real_transfers = False
            d_cplx = delta(lambda: sv.run_program(prog, th))   # the same plan forward on complex amplitudes
            sv.real_storage = sv.real_transfers = True
            got = []
            d_grad = delta(lambda: got.append(sv.program_energy_gradient(prog, th)))
            e, grad = got[0]
            counters = dict(getattr(sv.engine, "counters", {}))
            full = np.asarray(sv.gather_state())
            sv.free_plan(prog["ham"])
            res.append(dict(case=case, even=even, real=bool(prog["real"]), exchange_bits=list(prog["exchange_bits"]), swaps=prog["swaps"],
                            e=e, grad=grad, full=full, d_fwd=d_fwd, d_cplx=d_cplx, d_grad=d_grad, counters=counters,
                            chunks=same_x_chunks(prog), n_local=sv.n_local))
        if rank == 0:
            out.put(res)
    finally:
        dist.destroy_process_group()


def launch(target, world, args, timeout=600):
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port) + tuple(args[:2]) + (out,) + tuple(args[2:])) for r in range(world)]
    for p in procs:
        p.start()
    res = out.get(timeout=timeout)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return res


def check_gradient_cases(res, world, n):
    assert [r["even"] for r in res] == [False, True] and res[0]["real"] and not res[1]["real"]
    for r in res:
        c = r["case"]
        ew, gw = masks.ucc_energy_gradient(n, c["hf"], c["xs"], c["zs"], c["coeff"], c["pidx"], c["theta"], c["hx"], c["hz"], c["hc"],
                                           c["const"], phi0=c["phi0"])
        l1 = float(np.abs(c["hc"]).sum())
        de, dg = abs(r["e"] - ew), float(np.abs(r["grad"] - gw).max())
        print(f"world {world} n {n} even {r['even']}: exchange_bits {r['exchange_bits']} |dE|/|H|_1 {de / l1:.2e} "
              f"max|dgrad|/|H|_1 {dg / l1:.2e} max|grad| {np.abs(gw).max():.3f}")
        assert np.abs(gw).max() > 1e-2                              # (a gradient worth the name)
        assert de < BOUND * l1 and dg < BOUND * l1
        hf_state = np.zeros(1 << n, complex)
        hf_state[c["hf"]] = 1
        assert np.abs(r["full"] - hf_state).max() < 1e-12           # psi is back at |hf>
        # the backward pass: exactly the plan's exchanges, each moving psi AND lambda as complex amplitudes
        assert r["swaps"] >= 1 and r["d_cplx"]["swaps"] == r["swaps"]
        assert r["d_grad"]["swaps"] - r["d_fwd"]["swaps"] == r["swaps"]
        assert r["d_grad"]["bytes_sent"] - r["d_fwd"]["bytes_sent"] == 2 * r["d_cplx"]["bytes_sent"] > 0
        if world >= 4:
            assert max(r["exchange_bits"]) >= 2                     # multi-bit exchanges were replayed, not only half-shard ones


@pytest.mark.parametrize("world,n", [(2, 7), (4, 8), (8, 9)])
def test_adjoint_gradient_on_the_sharded_register(world, n):
    check_gradient_cases(launch(gradient_worker, world, (n, 31 + n)), world, n)


# ---- through the public face -------------------------------------------------------------------------------------------------------
def run_api(flows):
    """UCCEvaluator.energy_gradient and a short EnergyUCC._minimize with adjoint_gradient on whatever backend the process is set up for"""
    from openvqe_amd import chem, pools
    from openvqe_amd.evaluator import UCCEvaluator
    from openvqe_amd.ucc_family.get_energy_ucc import EnergyUCC
    mol = chem.molecule("H2")
    mol.rhf()
    ham = mol.jw_hamiltonian()
    _, pool = pools.spin_complement_gsd(mol.n_elec, mol.nao)
    hf = mol.hf_init()
    gens = [complex(0.0, 1.0) * pool[k] for k in (38, 32, 29, 23, 2)]     # Hermitian generators 1j * (T - T^+)
    out = {"l1": float(sum(abs(complex(t.coeff)) for t in ham.terms))}
    with contextlib.redirect_stdout(io.StringIO()):
        if "gradient" in flows:
            ev = UCCEvaluator(ham, gens, hf)
            theta = np.array([0.05, -0.02, 0.11, 0.3, -0.2])
            e, grad = ev.energy_gradient(theta)
            out["gradient"] = (float(e), np.asarray(grad), float(ev.energy(theta)))    # (the register serves energies again afterwards)
        if "minimize" in flows:
            ucc = EnergyUCC()
            ucc.adjoint_gradient = True
            energies = []
            res = ucc._minimize(ham, gens[:3], hf, [0.0, 0.0, 0.0], energies, "BFGS", 1e-4)
            out["minimize"] = (float(res.fun), np.asarray(res.x), len(energies))
    return out


def _reset():
    import openvqe_amd.evaluator as ev
    import openvqe_amd.qat_compat as qc
    ev._BACKENDS.clear()
    ev._Evaluator._owner.clear()
    qc._default_qpu = None


def api_worker(rank, world, port, engine, flows, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["OVQE_PARTITION_MIN_QUBITS"] = "6"
    os.environ["OVQE_SHARD_CHUNK_BITS"] = "3"
    os.environ["OVQE_SINGLE_DEVICE"] = "1"          # (HIP engine: every rank's shard on device 0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import openvqe_amd.evaluator as ev
        import openvqe_amd.partitioned as part
        if engine == "oracle":
            part.ENGINE_FACTORY = lambda nl, ng, r: AdjointOracleEngine(nl, ng, r)
        _reset()
        res = run_api(flows)
        from openvqe_amd.partitioned import PartitionedStatevector
        assert ev._BACKENDS and all(isinstance(sv, PartitionedStatevector) for sv in ev._BACKENDS.values())
        if rank == 0:
            out.put(res)
    finally:
        dist.destroy_process_group()


def single_process_api(flows):
    import openvqe_amd.backend as be
    import openvqe_amd.evaluator as ev
    saved = (be.Statevector, ev.Statevector)
    be.Statevector = ev.Statevector = AnalyticOracleStatevector
    _reset()
    try:
        return run_api(flows)
    finally:
        be.Statevector, ev.Statevector = saved
        _reset()


def check_api(got, want):
    l1 = want["l1"]
    (ge, gg, ge2), (we, wg, _) = got["gradient"], want["gradient"]
    print(f"|dE|/|H|_1 {abs(ge - we) / l1:.2e} max|dgrad|/|H|_1 {np.abs(gg - wg).max() / l1:.2e}")
    assert gg.shape == wg.shape == (5,) and np.abs(wg).max() > 1e-2
    assert abs(ge - we) < BOUND * l1 and np.abs(gg - wg).max() < BOUND * l1 and abs(ge2 - we) < BOUND * l1
    (gf, gx, gn), (wf, wx, wn) = got["minimize"], want["minimize"]
    # the same BFGS on gradients equal to rounding: same end point, far inside the optimiser's tolerance (1e-4)
    assert abs(gf - wf) < 1e-6 and np.abs(gx - wx).max() < 1e-4 and gn > 2


@pytest.mark.parametrize("world", [2, 4])
def test_adjoint_gradient_through_the_evaluator_on_the_partitioned_register(world):
    flows = ("gradient", "minimize")
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=api_worker, args=(r, world, port, "oracle", flows, out)) for r in range(world)]
    for p in procs:
        p.start()
    got = out.get(timeout=900)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    check_api(got, single_process_api(flows))
