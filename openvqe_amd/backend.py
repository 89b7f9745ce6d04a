"""Python face of the HIP statevector backend (one object == one ``ovqe_handle``).

Everything numerical happens in ``libovqe_sv.so``; this module only packs the reference's
operator objects (``.terms[i].{coeff,op,qbits}``) into the mask arrays of
``include/ovqe_sv.h`` and forwards.  No CPU implementation lives here.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import _lib
from .operators import pack_string, pack_terms

GATE_OPCODES = {"X": 0, "H": 1, "RX": 2, "RY": 3, "RZ": 4, "CNOT": 5}
GRAD_FERMIONIC, GRAD_QUBIT = 0, 1
_REAL_TOL = 1e-12


def _real_coeff(c, what):
    c = complex(c)
    if abs(c.imag) > _REAL_TOL * max(1.0, abs(c.real)):
        raise ValueError(f"{what}: Pauli coefficient {c} is not real (generator must be Hermitian — "
                         "multiply the anti-Hermitian cluster operator by 1j, ref:openvqe/algorithms/ucc.py:30-31)")
    return c.real


def compile_ucc_program(nbqbits, generators, n_params=None):
    """Flatten ``for op_k, theta_k: build_ucc_ansatz([op_k], ...)([theta_k])``
    (ref:openvqe/ucc_family/get_energy_ucc.py:42-45) into rotation arrays: rotation (k, j) is
    exp(-i theta_k c_kj P_kj), k outer / j in ``terms`` order (one Trotter step)."""
    K = len(generators) if n_params is None else min(len(generators), int(n_params))  # zip truncation
    counts = [len(generators[k].terms) for k in range(K)]
    terms = [term for k in range(K) for term in generators[k].terms]
    xs, zs, cc = pack_terms(nbqbits, terms)
    ps = np.repeat(np.arange(K, dtype=np.int32), counts)
    bad = np.abs(cc.imag) > _REAL_TOL * np.maximum(1.0, np.abs(cc.real))
    if bad.any():
        j = int(np.argmax(bad))
        _real_coeff(cc[j], f"generator {int(ps[j])}")   # raises with the reference's hint
    return xs, zs, np.ascontiguousarray(cc.real), ps, K


class Statevector:
    """n-qubit complex128 state resident on one MI355X (or one shard of a distributed state)."""

    def __init__(self, n_qubits, device=0, n_global=0, shard_index=0, view_of=None):
        """``view_of``: device pointer of a caller-owned buffer of 2^n_qubits amplitudes that IS the state (ovqe_create_view: no
        allocation of that size; the buffer must outlive the object)"""
        self._L = _lib.lib()
        self._h = ctypes.c_void_p()
        self._energy_io = None
        self.nbqbits = int(n_qubits) + int(n_global)
        self.n_local = int(n_qubits)
        self.n_global = int(n_global)
        self.shard_index = int(shard_index)
        self.device = int(device)
        if view_of is not None:
            if n_global:
                raise ValueError("a view is a single-device handle")
            rc = self._L.ovqe_create_view(n_qubits, device, ctypes.c_void_p(int(view_of)), ctypes.byref(self._h))
        elif n_global:
            rc = self._L.ovqe_create_shard(n_qubits, n_global, shard_index, device, ctypes.byref(self._h))
        else:
            rc = self._L.ovqe_create(n_qubits, device, ctypes.byref(self._h))
        if rc != 0:
            self._h = ctypes.c_void_p()
            _lib.check(rc, None)
        self._K = 0
        # OVQE_OPTIONS="name=value,name=value": tuning knobs (ovqe_set_option) for handles created inside library code —
        # the L1 mirrors and the qat stand-ins own their Statevector objects
        for item in os.environ.get("OVQE_OPTIONS", "").split(","):
            if "=" in item:
                name, value = item.split("=", 1)
                self.set_option(name.strip(), int(value))

    # -- lifecycle ------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.ovqe_destroy(self._h)
            self._h = ctypes.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _ck(self, rc):
        _lib.check(rc, self._h)

    def set_option(self, name, value):
        self._ck(self._L.ovqe_set_option(self._h, name.encode(), int(value)))

    def set_stream(self, hip_stream_handle):
        self._ck(self._L.ovqe_set_stream(self._h, ctypes.c_void_p(hip_stream_handle)))

    def adopt_state(self, device_ptr):
        self._ck(self._L.ovqe_adopt_state(self._h, ctypes.c_void_p(device_ptr)))

    def state_ptr(self):
        p = ctypes.c_void_p()
        self._ck(self._L.ovqe_state_ptr(self._h, ctypes.byref(p)))
        return p.value

    # -- state ----------------------------------------------------------------------------------
    def init_basis(self, index):
        self._ck(self._L.ovqe_init_basis(self._h, int(index)))

    def set_state(self, psi):
        psi = np.ascontiguousarray(psi, dtype=np.complex128)
        if psi.shape != (1 << self.n_local,):
            raise ValueError("state has the wrong length")
        self._ck(self._L.ovqe_set_state(self._h, psi.view(np.float64)))

    def get_state(self):
        out = np.empty(1 << self.n_local, dtype=np.complex128)
        self._ck(self._L.ovqe_get_state(self._h, out.view(np.float64)))
        return out

    def get_amplitudes(self, local_indices):
        idx = np.ascontiguousarray(local_indices, dtype=np.uint64)
        out = np.empty(idx.shape[0], dtype=np.complex128)
        self._ck(self._L.ovqe_get_amplitudes(self._h, idx.shape[0], idx, out.view(np.float64)))
        return out

    def randomize(self, seed, norm2_total=0.0):
        scale = ctypes.c_double()
        self._ck(self._L.ovqe_randomize(self._h, int(seed), float(norm2_total), ctypes.byref(scale)))
        return scale.value

    def norm2(self):
        out = ctypes.c_double()
        self._ck(self._L.ovqe_norm2(self._h, ctypes.byref(out)))
        return out.value

    # -- unit operations ------------------------------------------------------------------------
    def apply_pauli_rotation(self, x, z, phi):
        self._ck(self._L.ovqe_apply_pauli_rotation(self._h, int(x), int(z), float(phi)))

    def apply_pauli_rotations(self, xs, zs, phis):
        xs = np.ascontiguousarray(xs, np.uint64)
        zs = np.ascontiguousarray(zs, np.uint64)
        phis = np.ascontiguousarray(phis, np.float64)
        self._ck(self._L.ovqe_apply_pauli_rotations(self._h, xs.shape[0], xs, zs, phis))

    def adjoint_rotations(self, lam_ptr, xs, zs, phis):
        """backward step of the adjoint method (ovqe_adjoint_rotations): the rotations (forward order, local physical masks) are
        un-applied last to first from the state and from the 2^n_local complex amplitudes at device pointer ``lam_ptr``
        -> w[r] = Im <lam|P_r|psi> over this handle's amplitudes on the states after rotation r"""
        xs = np.ascontiguousarray(xs, np.uint64)
        zs = np.ascontiguousarray(zs, np.uint64)
        phis = np.ascontiguousarray(phis, np.float64)
        w = np.zeros(xs.shape[0], np.float64)
        self._ck(self._L.ovqe_adjoint_rotations(self._h, ctypes.c_void_p(int(lam_ptr)), xs.shape[0], xs, zs, phis, w))
        return w

    def rotate(self, op, qbits, phi):
        """exp(-i phi P) with P given as (pauli string, reference qubit list)."""
        x, z = pack_string(self.nbqbits, op, qbits)
        self.apply_pauli_rotation(x, z, phi)

    def apply_gate(self, name, qubits, angle=0.0):
        """literal gate on reference qubit indices (ref:openvqe/common_files/circuit.py gate set)."""
        n = self.nbqbits
        b0 = n - 1 - int(qubits[0])
        b1 = n - 1 - int(qubits[1]) if len(qubits) > 1 else 0
        self._ck(self._L.ovqe_apply_gate(self._h, GATE_OPCODES[name], b0, b1, float(angle or 0.0)))

    def expectation(self, hamiltonian):
        """Re <psi|H|psi> (+ constant) — the OBS job value (get_energy_ucc.py:46-48)."""
        xs, zs, cs = pack_terms(self.nbqbits, hamiltonian.terms)
        coeff = np.array([_real_coeff(c, "observable") for c in cs], np.float64)
        out = ctypes.c_double()
        const = _real_coeff(getattr(hamiltonian, "constant_coeff", 0.0) or 0.0, "observable constant")
        self._ck(self._L.ovqe_expectation(self._h, xs.shape[0], xs, zs, coeff, const, ctypes.byref(out)))
        return out.value

    def bilinear(self, xs, zs, coeff, bra_ptr=None, ket_ptr=None):
        coeff = np.asarray(coeff, np.complex128)
        out = np.zeros(2, np.float64)
        self._ck(self._L.ovqe_bilinear(self._h, ctypes.c_void_p(bra_ptr), ctypes.c_void_p(ket_ptr), len(xs),
                                       np.ascontiguousarray(xs, np.uint64), np.ascontiguousarray(zs, np.uint64),
                                       np.ascontiguousarray(coeff.real), np.ascontiguousarray(coeff.imag), out))
        return complex(out[0], out[1])

    def apply_pauli_sum(self, xs, zs, coeff, out_ptr, ket_ptr=None, accumulate=False):
        """out (+)= sum_t c_t P_t ket on explicit device buffers (ket None = the resident state); masks may carry one
        global x part when ket is the partner's shard"""
        coeff = np.asarray(coeff, np.complex128)
        self._ck(self._L.ovqe_apply_pauli_sum(self._h, ctypes.c_void_p(ket_ptr), ctypes.c_void_p(out_ptr), len(xs),
                                              np.ascontiguousarray(xs, np.uint64), np.ascontiguousarray(zs, np.uint64),
                                              np.ascontiguousarray(coeff.real), np.ascontiguousarray(coeff.imag),
                                              1 if accumulate else 0))

    def bilinear_batch(self, offsets, xs, zs, coeff, bra_ptr=None, ket_ptr=None):
        """[sum_{j in op k} c_j <bra|P_j|ket>] for every operator k, one launch -> complex array"""
        coeff = np.asarray(coeff, np.complex128)
        n_ops = len(offsets) - 1
        out = np.zeros(2 * max(n_ops, 1), np.float64)
        self._ck(self._L.ovqe_bilinear_batch(self._h, ctypes.c_void_p(bra_ptr), ctypes.c_void_p(ket_ptr), n_ops,
                                             np.ascontiguousarray(offsets, np.int64),
                                             np.ascontiguousarray(xs if len(xs) else [0], np.uint64),
                                             np.ascontiguousarray(zs if len(zs) else [0], np.uint64),
                                             np.ascontiguousarray(coeff.real if len(coeff) else [0.0]),
                                             np.ascontiguousarray(coeff.imag if len(coeff) else [0.0]), out))
        return out[0:2 * n_ops:2] + 1j * out[1:2 * n_ops:2]

    # -- Pauli sums planned once for a shard of the partitioned register (ovqe_xsum_*, csrc/cross_host.inc) -------------------
    def xsum_create(self, xs, zs, coeff, chunk_bits):
        """plan of sum_t c_t P_t (masks in the physical index-bit space of the WHOLE register) on this shard -> id"""
        coeff = np.asarray(coeff, np.complex128)
        sid = ctypes.c_int32()
        n = len(xs)
        one = np.zeros(1)
        self._ck(self._L.ovqe_xsum_create(self._h, n, np.ascontiguousarray(xs if n else [0], np.uint64),
                                          np.ascontiguousarray(zs if n else [0], np.uint64),
                                          np.ascontiguousarray(coeff.real) if n else one,
                                          (np.ascontiguousarray(coeff.imag) if n else one) if np.any(coeff.imag != 0.0) else None,
                                          int(chunk_bits), ctypes.byref(sid)))
        return sid.value

    def xsum_destroy(self, sid):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.ovqe_xsum_destroy(self._h, int(sid))

    def xsum_partners(self, sid):
        """[(rank difference d, passes one chunk of that partner costs)]"""
        n = ctypes.c_int64()
        self._ck(self._L.ovqe_xsum_partners(self._h, int(sid), 0, None, None, ctypes.byref(n)))
        d, p = np.zeros(max(n.value, 1), np.uint64), np.zeros(max(n.value, 1), np.int64)
        self._ck(self._L.ovqe_xsum_partners(self._h, int(sid), n.value, d.ctypes.data, p.ctypes.data, ctypes.byref(n)))
        return [(int(d[k]), int(p[k])) for k in range(n.value)]

    def xsum_info(self, sid):
        out = (ctypes.c_int64 * 10)()
        self._ck(self._L.ovqe_xsum_info(self._h, int(sid), out, 10))
        keys = ("local_groups", "local_terms", "local_tile_sweeps", "local_untiled_groups", "partners", "remote_groups",
                "remote_terms", "remote_passes_per_chunk", "tile_bits", "streaming_fallback")
        return dict(zip(keys, [int(v) for v in out]))

    def xsum_expect_local(self, sid):
        out = ctypes.c_double()
        self._ck(self._L.ovqe_xsum_expect_local(self._h, int(sid), ctypes.byref(out)))
        return out.value

    def xsum_expect_remote(self, sid, d, chunk, ket_ptr):
        self._ck(self._L.ovqe_xsum_expect_remote(self._h, int(sid), int(d), int(chunk), ctypes.c_void_p(ket_ptr)))

    # -- the ADAPT pool planned once for a shard of the partitioned register (ovqe_xpool_*, csrc/pool_host.inc) ---------------------
    def xpool_create(self, offsets, xs, zs, coeff, chunk_bits):
        """plan of the pool operators A_k = sum_{t in [offsets[k], offsets[k + 1])} c_t P_t (physical masks of the WHOLE register) -> id"""
        coeff = np.asarray(coeff, np.complex128).reshape(-1)
        offsets = np.ascontiguousarray(offsets, np.int64)
        pid = ctypes.c_int32()
        n = len(xs)
        one = np.zeros(1)
        self._ck(self._L.ovqe_xpool_create(self._h, len(offsets) - 1, offsets, np.ascontiguousarray(xs if n else [0], np.uint64),
                                           np.ascontiguousarray(zs if n else [0], np.uint64),
                                           np.ascontiguousarray(coeff.real) if n else one,
                                           (np.ascontiguousarray(coeff.imag) if n else one) if np.any(coeff.imag != 0.0) else None,
                                           int(chunk_bits), ctypes.byref(pid)))
        self.__dict__.setdefault("_xpool_ops", {})[pid.value] = len(offsets) - 1
        return pid.value

    def xpool_destroy(self, pid):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.ovqe_xpool_destroy(self._h, int(pid))

    def xpool_partners(self, pid):
        """[(rank difference d, passes one chunk of that partner costs)]"""
        n = ctypes.c_int64()
        self._ck(self._L.ovqe_xpool_partners(self._h, int(pid), 0, None, None, ctypes.byref(n)))
        d, p = np.zeros(max(n.value, 1), np.uint64), np.zeros(max(n.value, 1), np.int64)
        self._ck(self._L.ovqe_xpool_partners(self._h, int(pid), n.value, d.ctypes.data, p.ctypes.data, ctypes.byref(n)))
        return [(int(d[k]), int(p[k])) for k in range(n.value)]

    def xpool_info(self, pid):
        out = (ctypes.c_int64 * 9)()
        self._ck(self._L.ovqe_xpool_info(self._h, int(pid), out, 9))
        keys = ("operators", "entries", "x_masks", "partners", "remote_passes_per_chunk", "local_passes", "tile_bits",
                "streaming_fallback", "partial_bytes")
        return dict(zip(keys, [int(v) for v in out]))

    def xpool_local(self, pid, bra_ptr):
        self._ck(self._L.ovqe_xpool_local(self._h, int(pid), ctypes.c_void_p(bra_ptr)))

    def xpool_remote(self, pid, d, chunk, ket_ptr, bra_ptr):
        self._ck(self._L.ovqe_xpool_remote(self._h, int(pid), int(d), int(chunk), ctypes.c_void_p(ket_ptr), ctypes.c_void_p(bra_ptr)))

    def xpool_finish(self, pid):
        """v_k per operator (complex array) since the last finish; resets the accumulators"""
        n_ops = self._xpool_ops[int(pid)]
        out = np.zeros(2 * max(n_ops, 1), np.float64)
        self._ck(self._L.ovqe_xpool_finish(self._h, int(pid), out))
        return out[0:2 * n_ops:2] + 1j * out[1:2 * n_ops:2]

    # -- k-bit shard exchange: one block of the shard <-> a contiguous stream (ovqe_shard_pack / ovqe_shard_unpack; enqueue only) ----
    def shard_pack(self, local_bit_mask, block, first, count, dst_ptr, real_parts_only=False):
        """dst[j - first] = amplitude j of block ``block`` of the local bits ``local_bit_mask``, j in [first, first + count)"""
        self._ck(self._L.ovqe_shard_pack(self._h, int(local_bit_mask), int(block), int(first), int(count), ctypes.c_void_p(dst_ptr),
                                         1 if real_parts_only else 0))

    def shard_unpack(self, local_bit_mask, block, first, count, src_ptr, real_parts_only=False):
        """the inverse scatter of ``shard_pack`` (real parts only: the imaginary parts become exact zeros)"""
        self._ck(self._L.ovqe_shard_unpack(self._h, int(local_bit_mask), int(block), int(first), int(count), ctypes.c_void_p(src_ptr),
                                           1 if real_parts_only else 0))

    def xsum_expect_finish(self, sid):
        out = np.zeros(2, np.float64)
        self._ck(self._L.ovqe_xsum_expect_finish(self._h, int(sid), out))
        return complex(out[0], out[1])

    def xsum_apply_local(self, sid, out_ptr, ident=0.0):
        self._ck(self._L.ovqe_xsum_apply_local(self._h, int(sid), ctypes.c_void_p(out_ptr), float(ident)))

    # -- Lanczos vector operations on device buffers of the handle's storage (shard-local partials; ovqe_vec_*)
    def vec_dot(self, a_ptr, b_ptr):
        out = np.zeros(2, np.float64)
        self._ck(self._L.ovqe_vec_dot(self._h, ctypes.c_void_p(a_ptr), ctypes.c_void_p(b_ptr), out))
        return complex(out[0], out[1])

    def vec_lanczos_update(self, w_ptr, v_ptr, vprev_ptr, alpha, beta):
        out = ctypes.c_double()
        self._ck(self._L.ovqe_vec_lanczos_update(self._h, ctypes.c_void_p(w_ptr), ctypes.c_void_p(v_ptr),
                                                 None if vprev_ptr is None else ctypes.c_void_p(vprev_ptr), float(alpha), float(beta),
                                                 ctypes.byref(out)))
        return out.value

    def vec_scale(self, v_ptr, s):
        self._ck(self._L.ovqe_vec_scale(self._h, ctypes.c_void_p(v_ptr), float(s)))

    def vec_axpy(self, y_ptr, x_ptr, s, overwrite=False):
        self._ck(self._L.ovqe_vec_axpy(self._h, ctypes.c_void_p(y_ptr), ctypes.c_void_p(x_ptr), float(s), 1 if overwrite else 0))

    def xsum_apply_remote(self, sid, d, chunk, ket_ptr, out_ptr):
        self._ck(self._L.ovqe_xsum_apply_remote(self._h, int(sid), int(d), int(chunk), ctypes.c_void_p(ket_ptr),
                                                ctypes.c_void_p(out_ptr)))

    # -- compiled evaluation --------------------------------------------------------------------
    def set_hamiltonian(self, hamiltonian):
        xs, zs, cs = pack_terms(self.nbqbits, hamiltonian.terms)
        coeff = np.array([_real_coeff(c, "observable") for c in cs], np.float64)
        const = _real_coeff(getattr(hamiltonian, "constant_coeff", 0.0) or 0.0, "observable constant")
        self._ck(self._L.ovqe_set_hamiltonian(self._h, xs.shape[0], xs, zs, coeff, const))
        self._ham_terms = int(xs.shape[0])
        self._ham_norm1 = float(np.abs(coeff).sum())

    def hamiltonian_norm1(self):
        """sum_t |c_t| of the stored Hamiltonian, without its constant: a bound on its spectral radius"""
        if getattr(self, "_ham_norm1", None) is None:
            raise RuntimeError("no Hamiltonian set")
        return self._ham_norm1

    def set_rotation_program(self, xs, zs, coeffs, pidx, n_params, hf_init, phi0=None):
        xs = np.ascontiguousarray(xs, np.uint64)
        self._ck(self._L.ovqe_set_program(self._h, xs.shape[0], xs, np.ascontiguousarray(zs, np.uint64),
                                          np.ascontiguousarray(coeffs, np.float64),
                                          None if phi0 is None else np.ascontiguousarray(phi0, np.float64),
                                          np.ascontiguousarray(pidx, np.int32), int(n_params), int(hf_init)))
        self._K = int(n_params)

    def set_ucc_program(self, generators, hf_init, n_params=None):
        xs, zs, cs, ps, K = compile_ucc_program(self.nbqbits, generators, n_params)
        self.set_rotation_program(xs, zs, cs, ps, K, hf_init)
        return K

    def set_gate_program(self, gates, n_params, hf_init):
        """gates: list of (name, qubits, angle_scale, angle_const, param_index or -1)."""
        n = self.nbqbits
        G = len(gates)
        opc = np.zeros(G, np.int32)
        b0 = np.zeros(G, np.int32)
        b1 = np.zeros(G, np.int32)
        asc = np.zeros(G, np.float64)
        aco = np.zeros(G, np.float64)
        pid = np.full(G, -1, np.int32)
        for g, (name, qubits, scale, const, p) in enumerate(gates):
            opc[g] = GATE_OPCODES[name]
            b0[g] = n - 1 - int(qubits[0])
            b1[g] = n - 1 - int(qubits[1]) if len(qubits) > 1 else 0
            asc[g], aco[g], pid[g] = scale, const, p
        self._ck(self._L.ovqe_set_gate_program(self._h, G, opc, b0, b1, asc, aco, pid, int(n_params), int(hf_init)))
        self._K = int(n_params)

    def energy(self, theta):
        K = self._K
        io = self._energy_io
        if io is None or io[0].shape[0] != max(K, 1):   # parameter buffer + result slot of this handle, their addresses taken once
            buf = np.zeros(max(K, 1), np.float64)
            out = ctypes.c_double()
            io = self._energy_io = (buf, out, ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(ctypes.addressof(out)))
        buf, out, buf_p, out_p = io
        theta = np.asarray(theta, np.float64).reshape(-1)
        if theta.shape[0] < K:
            raise ValueError(f"expected {K} parameters")
        buf[:K] = theta[:K]
        rc = self._L.ovqe_energy_raw(self._h, buf_p, K, out_p)
        if rc:
            self._ck(rc)
        return out.value

    def energy_batch(self, thetas):
        thetas = np.ascontiguousarray(thetas, np.float64)
        if thetas.ndim != 2 or thetas.shape[1] != self._K:
            raise ValueError(f"expected a (B, {self._K}) array")
        out = np.empty(thetas.shape[0], np.float64)
        self._ck(self._L.ovqe_energy_batch(self._h, thetas.shape[0], thetas if thetas.size else np.zeros(1),
                                           self._K, out))
        return out

    def energy_batch_device(self, n_batch, theta_ptr, energies_ptr):
        """B evaluations with theta (B x K float64, row-major) and energies (B float64) resident on the device —
        e.g. ``tensor.data_ptr()`` of torch CUDA tensors; returns when the energies are written."""
        self._ck(self._L.ovqe_energy_batch_device(self._h, int(n_batch), ctypes.c_void_p(theta_ptr), self._K,
                                                  ctypes.c_void_p(energies_ptr)))

    def prepare_state(self, theta):
        theta = np.ascontiguousarray(theta, np.float64).reshape(-1)[: self._K]
        self._ck(self._L.ovqe_prepare_state(self._h, theta if self._K else np.zeros(1), self._K))

    def last_batch_ms(self):
        out = ctypes.c_double()
        self._ck(self._L.ovqe_last_batch_ms(self._h, ctypes.byref(out)))
        return out.value

    def get_support(self, capacity=None):
        """(indices, amplitudes) of the non-zero amplitudes, ascending index, listed on the device — or None when the
        list is not available (register below 12 qubits, shard of a distributed register) or longer than ``capacity``
        (default: 1/8 of the register)"""
        cap = int(capacity if capacity is not None else max(1, (1 << self.n_local) // 8))
        idx = np.empty(cap, np.uint64)
        amp = np.empty(cap, np.complex128)
        count = ctypes.c_int64()
        self._ck(self._L.ovqe_get_support(self._h, cap, idx.ctypes.data, amp.ctypes.data, ctypes.byref(count)))
        if count.value < 0 or count.value > cap:
            return None
        return idx[:count.value].copy(), amp[:count.value].copy()

    def last_screen_support(self):
        """non-zero amplitudes the last ``pool_gradients`` call walked instead of the register (-1: the register)"""
        out = ctypes.c_int64()
        self._ck(self._L.ovqe_last_support(self._h, 0, ctypes.byref(out)))
        return out.value

    def last_screen_sector(self):
        """determinants of the symmetry sector whose materialised Hamiltonian gave sigma = H psi of the last ``pool_gradients``
        call (0: sigma from the register / the tile cover)"""
        out = ctypes.c_int64()
        self._ck(self._L.ovqe_last_support(self._h, 2, ctypes.byref(out)))
        return out.value

    def last_fci_rounds(self):
        """matrix-vector rounds the last ``sector_ground_state`` call needed to saturate the block of H connected to the
        reference determinant"""
        out = ctypes.c_int64()
        self._ck(self._L.ovqe_last_support(self._h, 3, ctypes.byref(out)))
        return out.value

    def last_passes(self):
        """(passes over the state, bytes they move by construction) of the last ``apply_pauli_rotations`` / ``bilinear`` /
        ``expectation`` call"""
        a, b = ctypes.c_int64(), ctypes.c_int64()
        self._ck(self._L.ovqe_last_support(self._h, 4, ctypes.byref(a)))
        self._ck(self._L.ovqe_last_support(self._h, 5, ctypes.byref(b)))
        return a.value, b.value

    SECTOR_FORMS = ("sweep_pairs", "sweep_wide", "sweep_streams", "sweep_regular", "adjoint_pairs", "adjoint_wide", "adjoint_streams",
                    "adjoint_regular", "pair_builder_first", "pair_builder_staged")

    def sector_forms(self):
        """names of the sector-path kernel forms that served this handle since its program was set (ovqe_last_support, which = 6)"""
        out = ctypes.c_int64()
        self._ck(self._L.ovqe_last_support(self._h, 6, ctypes.byref(out)))
        return {name for bit, name in enumerate(self.SECTOR_FORMS) if (out.value >> bit) & 1}

    #: the choices inside a sector kernel form, bits 10... of the same word (ovqe_sv.hip: SECF_*), set where the kernel is launched
    SECTOR_CHOICES = ("sweep_pairs_ahead", "sweep_pairs_plain", "scatter_in_lds", "scatter_late", "pair_builder_dense_map",
                      "pair_builder_search", "apply_atomic", "apply_sequential", "apply_512", "apply_1024",
                      "h_packed24", "h_dict32", "h_explicit_overflow", "h_explicit_sample_failed", "h_explicit_no_dict") + tuple(
                          f"{group}_{nt}" for group in ("sweep", "adjoint", "regular") for nt in (64, 128, 256, 512, 1024))

    def sector_choices(self):
        """what the sector-path kernels of ``sector_forms()`` were launched as on this handle since its program was set: the staging
        variant of the first sweep form ("sweep_pairs_ahead": k_sector_sweep<NT, true>), where the second and third forms keep their
        scatter indices, the slot map of the pair-table builder, store mode and workgroup size of lambda = H psi (k_sector_apply),
        the coding outcomes of the materialised <H> (one name per outcome that at least one sweep took) and the workgroup sizes of
        the circuit sweeps ("sweep_256"), the backward sweeps ("adjoint_1024") and the regular-support sweeps ("regular_128").
        ``sector_forms()`` keeps returning the form names alone."""
        out = ctypes.c_int64()
        self._ck(self._L.ovqe_last_support(self._h, 6, ctypes.byref(out)))
        return {name for bit, name in enumerate(self.SECTOR_CHOICES) if (out.value >> (10 + bit)) & 1}

    SPARSE_FORMS = ("wg","staged1", "plain1", "rows2", "plain2", "plain4", "grad_wg", "grad_staged", "grad_plain", "declined")

    def sparse_forms(self):
        """names of the support-compacted kernel forms that served this handle since its program was set (ovqe_last_support,
        which = 7); "declined": a call that wanted the compact path was served by the other paths"""
        out = ctypes.c_int64()
        self._ck(self._L.ovqe_last_support(self._h, 7, ctypes.byref(out)))
        return {name for bit, name in enumerate(self.SPARSE_FORMS) if (out.value >> bit) & 1}

    #: launch geometries of the "rows2" form, bits 10... of the same word (sparse_host.inc: SPG_*)
    SPARSE_GEOMETRIES = ("per_wave", "shared_e37_s4104", "shared_e13_s2568")

    def sparse_geometries(self):
        """launch geometries that served the "rows2" form on this handle since its program was set: "per_wave" (k_sparse_vqe_rows<2>,
        one wave per pair of evaluations) or an instance of the workgroup geometry with the Hamiltonian's entries in registers
        (k_sparse_vqe_rows_shared).  A name identifies the instance — "e37": it takes programs of up to 37 entries per thread,
        "s4104": bytes between the states in LDS — not the layout of the entries in the registers (owner pieces:
        ``program_info()["sp_h_slots"]``, ``["sp_h_reads_per_state"]``)"""
        out = ctypes.c_int64()
        self._ck(self._L.ovqe_last_support(self._h, 7, ctypes.byref(out)))
        return {name for bit, name in enumerate(self.SPARSE_GEOMETRIES) if (out.value >> (10 + bit)) & 1}

    def fused_launch(self):
        """the most recent launch of the fused whole-circuit kernel on this handle since its program was set (ovqe_last_support,
        which = 8..13) -> dict; ``launched`` is False, and every count 0, when there was none"""
        v = []
        for which in range(8, 14):
            out = ctypes.c_int64()
            self._ck(self._L.ovqe_last_support(self._h, which, ctypes.byref(out)))
            v.append(out.value)
        bits = v[0]
        return {"launched": v[1] > 0, "real": bool(bits & 1), "lds_state": bool(bits & 2), "threads": (64, 256, 1024, 0)[(bits >> 2) & 3],
                "mapped_io": bool(bits & 16), "polled": bool(bits & 32), "device_entry": bool(bits & 64), "form_bits": bits,
                "workgroups": v[1], "segments": v[2], "exp_chunks": v[3], "exp_entries": v[4], "flat_items": v[5]}

    def last_exp_support(self):
        """amplitudes the Taylor steps of the last ``apply_exp_pauli_sum`` call ran over (-1: the register)"""
        out = ctypes.c_int64()
        self._ck(self._L.ovqe_last_support(self._h, 1, ctypes.byref(out)))
        return out.value

    def energy_gradient(self, theta):
        """E(theta) and the exact gradient dE/dtheta by the adjoint method (one forward + one backward pass over the
        program for all K derivatives) -> (energy, grad[K])"""
        theta = np.ascontiguousarray(theta, np.float64).reshape(-1)[: self._K]
        if theta.shape[0] != self._K:
            raise ValueError(f"expected {self._K} parameters")
        e = ctypes.c_double()
        grad = np.zeros(max(self._K, 1), np.float64)
        self._ck(self._L.ovqe_energy_gradient(self._h, theta if self._K else np.zeros(1), self._K, ctypes.byref(e), grad))
        return e.value, grad[: self._K]

    def energy_gradient_batch(self, thetas):
        """E and the exact gradient of every row of ``thetas`` (B, K) -> (energies[B], grads[B, K]); row b is what
        ``energy_gradient(thetas[b])`` answers.  A program on the compact support runs the whole batch in one launch
        (ovqe_energy_gradient_batch, csrc/gradbatch_host.inc; ``gradient_batch_info``), every other program row by row"""
        thetas = np.ascontiguousarray(thetas, np.float64)
        if thetas.ndim != 2 or thetas.shape[1] != self._K:
            raise ValueError(f"expected a (B, {self._K}) array")
        B, K = thetas.shape
        energies = np.zeros(B, np.float64)
        grads = np.zeros((B, K), np.float64)
        self._ck(self._L.ovqe_energy_gradient_batch(self._h, B, thetas if thetas.size else np.zeros(1), K, energies if B else np.zeros(1),
                                                    grads.reshape(-1) if grads.size else np.zeros(1)))
        return energies, grads

    def gradient_batch_info(self):
        """figures of the last ``energy_gradient_batch`` call: path (1 compact support in one launch, 2 row by row), rows, parameters,
        launches, kernel form (1 op records and pair words staged in LDS, 2 read from global memory, 0 on path 2), waves per workgroup,
        workgroups, dynamic LDS bytes, support size, and the HIP-event times in microseconds of the copy of theta with the launch and of
        the copy back"""
        out = (ctypes.c_int64 * 11)()
        self._ck(self._L.ovqe_gradient_batch_info(self._h, out, 11))
        keys = ("path", "B", "K", "launches", "form", "waves", "workgroups", "lds_bytes", "support", "launch_us", "copy_back_us")
        return dict(zip(keys, [int(v) for v in out]))

    # -- variational quantum deflation (ovqe_deflation_*, ovqe_deflated_gradient_batch, csrc/deflate_host.inc) ---------------------
    def deflation_push(self, beta):
        """the state in the buffer, as it is, becomes the next deflation vector phi_j of the handle with weight ``beta`` >= 0 (at most
        32; they survive a new program or Hamiltonian) -> the number of vectors held"""
        self._ck(self._L.ovqe_deflation_push(self._h, float(beta)))
        return self.deflation_count()

    def deflation_truncate(self, count=0):
        """keeps the first ``count`` deflation vectors, frees the rest (0: all of them)"""
        self._ck(self._L.ovqe_deflation_truncate(self._h, int(count)))

    def deflation_count(self):
        out = ctypes.c_int32()
        self._ck(self._L.ovqe_deflation_count(self._h, ctypes.byref(out)))
        return out.value

    def deflated_gradient_batch(self, thetas):
        """C = <H> + sum_j beta_j |<phi_j|psi>|^2 with the deflation vectors held, for every row of ``thetas`` (B, K)
        -> (costs[B], dC/dtheta[B, K], energies[B], overlaps[B, J] complex).  A program on the compact support runs the whole batch in
        one launch (``deflation_info``), every other program row by row on the streaming kernels"""
        thetas = np.ascontiguousarray(thetas, np.float64)
        if thetas.ndim != 2 or thetas.shape[1] != self._K:
            raise ValueError(f"expected a (B, {self._K}) array")
        B, K = thetas.shape
        J = self.deflation_count()
        costs, energies = np.zeros(B, np.float64), np.zeros(B, np.float64)
        grads = np.zeros((B, K), np.float64)
        overlaps = np.zeros((B, J), np.complex128)
        self._ck(self._L.ovqe_deflated_gradient_batch(
            self._h, B, thetas if thetas.size else np.zeros(1), K, costs if B else np.zeros(1), grads.reshape(-1) if grads.size else np.zeros(1),
            energies if B else np.zeros(1), overlaps.view(np.float64).reshape(-1) if overlaps.size else None))
        return costs, grads, energies, overlaps

    def deflation_info(self):
        """figures of the last ``deflated_gradient_batch`` call: path (1 compact support in one launch, 2 streaming), rows, parameters,
        vectors, real rows of path 1, launches, kernel form, waves per workgroup, workgroups, dynamic LDS bytes, support size, gather
        launches of the call (0: the cached rows served), and the HIP-event times in microseconds of the copy of theta with the launch
        and of the copy back"""
        out = (ctypes.c_int64 * 14)()
        self._ck(self._L.ovqe_deflation_info(self._h, out, 14))
        keys = ("path", "B", "K", "J", "rows", "launches", "form", "waves", "workgroups", "lds_bytes", "support", "gather_launches",
                "launch_us", "copy_back_us")
        return dict(zip(keys, [int(v) for v in out]))

    # -- energy spread: variance and folded-spectrum cost (ovqe_spread_gradient_batch, csrc/spread_host.inc) --------------------------
    def spread_gradient_batch(self, thetas, omega=None, w_energy=0.0, w_spread=1.0):
        """S = ||(H - omega) psi||^2 for every row of ``thetas`` (B, K): ``omega`` a scalar or B values — the folded-spectrum cost — or
        None for omega_b = E_b, where S is the energy variance <H^2> - <H>^2
        -> (costs[B] = w_energy E + w_spread S, d costs/dtheta[B, K] at fixed omega, energies[B], spreads[B]).  In variance mode the
        gradient is the exact gradient of w_energy E + w_spread Var.  A program on the compact support whose Hamiltonian stays on it
        runs the whole batch in one launch (``spread_info``), every other program row by row on the streaming kernels"""
        thetas = np.ascontiguousarray(thetas, np.float64)
        if thetas.ndim != 2 or thetas.shape[1] != self._K:
            raise ValueError(f"expected a (B, {self._K}) array")
        B, K = thetas.shape
        if omega is not None:
            omega = np.ascontiguousarray(np.broadcast_to(np.asarray(omega, np.float64), (B,)))
        costs, energies, spreads = np.zeros(B, np.float64), np.zeros(B, np.float64), np.zeros(B, np.float64)
        grads = np.zeros((B, K), np.float64)
        self._ck(self._L.ovqe_spread_gradient_batch(
            self._h, B, thetas if thetas.size else np.zeros(1), K, None if omega is None else (omega if B else np.zeros(1)),
            float(w_energy), float(w_spread), costs if B else np.zeros(1), grads.reshape(-1) if grads.size else np.zeros(1),
            energies if B else np.zeros(1), spreads if B else np.zeros(1)))
        return costs, grads, energies, spreads

    def energy_variance(self, theta):
        """-> (E, Var) at ``theta``: Var = <H^2> - <H>^2 = ||(H - E) psi||^2, zero exactly on eigenstates; an eigenvalue of H lies within
        sqrt(Var) of E"""
        _, _, e, s = self.spread_gradient_batch(np.asarray(theta, np.float64).reshape(1, -1))
        return float(e[0]), float(s[0])

    def spread_info(self):
        """figures of the last ``spread_gradient_batch`` call: path (1 compact support in one launch, 2 streaming), rows, parameters,
        mode (0 omega given, 1 variance), launches, kernel form, waves per workgroup, workgroups, dynamic LDS bytes, support size, why
        path 2 served it (0 it did not, 1 no compact program or options, 2 LDS, 3 the Hamiltonian leaks from the support, 4 a term with
        an odd number of Y), and the HIP-event times in microseconds of the copy of theta with the launch and of the copy back"""
        out = (ctypes.c_int64 * 13)()
        self._ck(self._L.ovqe_spread_info(self._h, out, 13))
        keys = ("path", "B", "K", "mode", "launches", "form", "waves", "workgroups", "lds_bytes", "support", "why", "launch_us",
                "copy_back_us")
        return dict(zip(keys, [int(v) for v in out]))

    # -- observables beside the Hamiltonian (ovqe_observable_*, ovqe_constrained_gradient_batch, csrc/constrain_host.inc) ------------
    def observable_push(self, hamiltonian):
        """the Hermitian Pauli sum ``hamiltonian`` (real coefficients) becomes the next observable O_m of the handle (at most 8; they
        survive a new program or Hamiltonian) -> the number of observables held"""
        xs, zs, cs = pack_terms(self.nbqbits, hamiltonian.terms)
        coeff = np.array([_real_coeff(c, "observable") for c in cs], np.float64)
        const = _real_coeff(getattr(hamiltonian, "constant_coeff", 0.0) or 0.0, "observable constant")
        self._ck(self._L.ovqe_observable_push(self._h, xs.shape[0], xs, zs, coeff, const))
        return self.observable_count()

    def observable_truncate(self, count=0):
        """keeps the first ``count`` observables, frees the rest (0: all of them)"""
        self._ck(self._L.ovqe_observable_truncate(self._h, int(count)))

    def observable_count(self):
        out = ctypes.c_int32()
        self._ck(self._L.ovqe_observable_count(self._h, ctypes.byref(out)))
        return out.value

    def constrained_gradient_batch(self, thetas, linear=None, quad=None, target=None):
        """C = <H> + sum_m [linear_m o_m + quad_m (o_m - target_m)^2] + sum_j beta_j |<phi_j|psi>|^2 with the observables and deflation
        vectors held, o_m = <psi|O_m|psi> with O_m's constant, for every row of ``thetas`` (B, K); ``linear``, ``quad``, ``target``: M
        values each or None for zeros
        -> (costs[B], dC/dtheta[B, K], energies[B], values[B, M], overlaps[B, J] complex).  A program on the compact support runs the
        whole batch in one launch (``constraint_info``), every other program row by row on the streaming kernels"""
        thetas = np.ascontiguousarray(thetas, np.float64)
        if thetas.ndim != 2 or thetas.shape[1] != self._K:
            raise ValueError(f"expected a (B, {self._K}) array")
        B, K = thetas.shape
        M, J = self.observable_count(), self.deflation_count()

        def weights(w, name):
            if w is None:
                return None
            w = np.ascontiguousarray(np.asarray(w, np.float64).reshape(-1))
            if w.shape[0] != M:
                raise ValueError(f"{name}: expected {M} values, one per observable held")
            return w if M else None
        linear, quad, target = weights(linear, "linear"), weights(quad, "quad"), weights(target, "target")
        costs, energies = np.zeros(B, np.float64), np.zeros(B, np.float64)
        grads = np.zeros((B, K), np.float64)
        values = np.zeros((B, M), np.float64)
        overlaps = np.zeros((B, J), np.complex128)
        self._ck(self._L.ovqe_constrained_gradient_batch(
            self._h, B, thetas if thetas.size else np.zeros(1), K, M, linear, quad, target, costs if B else np.zeros(1),
            grads.reshape(-1) if grads.size else np.zeros(1), energies if B else np.zeros(1),
            values.reshape(-1) if values.size else None, overlaps.view(np.float64).reshape(-1) if overlaps.size else None))
        return costs, grads, energies, values, overlaps

    def expectations_batch(self, thetas):
        """-> (energies[B], values[B, M]): <H> and the expectation values of the observables held for every row of ``thetas``"""
        _, _, energies, values, _ = self.constrained_gradient_batch(thetas)
        return energies, values

    def constraint_info(self):
        """figures of the last ``constrained_gradient_batch`` call: path (1 compact support in one launch, 2 streaming), rows,
        parameters, observables, vectors, real deflation rows of path 1, launches, kernel form, waves per workgroup, workgroups, dynamic
        LDS bytes, support size, entries of all restricted observables, observables restricted by the call (0: the cached entries
        served), and the HIP-event times in microseconds of the copy of theta with the launch and of the copy back"""
        out = (ctypes.c_int64 * 16)()
        self._ck(self._L.ovqe_constraint_info(self._h, out, 16))
        keys = ("path", "B", "K", "M", "J", "rows", "launches", "form", "waves", "workgroups", "lds_bytes", "support", "entries",
                "restriction_builds", "launch_us", "copy_back_us")
        return dict(zip(keys, [int(v) for v in out]))

    def ground_state(self, tol=1e-10, max_iter=3000, seed=20250227):
        """lowest eigenpair of the stored Hamiltonian by device-side Lanczos; the eigenvector is left in the
        state buffer (``get_state``).  -> (energy, residual |H y - E y|, iterations)"""
        e, r, it = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        self._ck(self._L.ovqe_ground_state(self._h, float(tol), int(max_iter), int(seed), ctypes.byref(e),
                                           ctypes.byref(r), ctypes.byref(it)))
        return e.value, r.value, it.value

    def sector_ground_state(self, tol=1e-10, max_iter=1000, seed=20250227):
        """lowest eigenpair of the stored Hamiltonian restricted to the support of the stored program's states (sector tables):
        the FCI energy of the Hartree-Fock determinant's symmetry sector for a number- and spin-conserving ansatz.
        -> (energy, residual |H y - E y|, iterations)"""
        e, r, it = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        self._ck(self._L.ovqe_sector_ground_state(self._h, float(tol), int(max_iter), int(seed), ctypes.byref(e),
                                                  ctypes.byref(r), ctypes.byref(it)))
        return e.value, r.value, it.value

    # -- reduced density matrices of the resident state (ovqe_rdm, csrc/rdm_host.inc) -------------------------------------------
    def rdm1(self):
        """gamma[p, q] = <a+_p a_q> of the resident state, (n, n) complex128: Jordan-Wigner, orbital p = qubit p, spin orbitals
        interleaved (even alpha, odd beta) — the conventions of ``fermion.spin_orbital_integrals``; helpers in ``openvqe_amd.rdm``"""
        n = self.n_local
        out = np.empty((n, n), np.complex128)
        self._ck(self._L.ovqe_rdm(self._h, 1, out.view(np.float64).reshape(-1)))
        return out

    def rdm2(self, packed=False):
        """Gamma[p, q, r, s] = <a+_p a+_q a_r a_s> of the resident state, (n, n, n, n) complex128 — so that E = constant +
        sum h_pq gamma_pq + 1/2 sum h_pqrs Gamma_pqrs with the integrals of ``fermion.spin_orbital_integrals`` — or, ``packed``,
        what the device computes: D2[(p<q), (r<s)] = <a+_p a+_q a_s a_r>, (P, P) with the P = n(n-1)/2 pairs in lexicographic order"""
        from . import rdm
        n = self.n_local
        P = n * (n - 1) // 2
        out = np.empty((P, P), np.complex128)
        self._ck(self._L.ovqe_rdm(self._h, 2, out.view(np.float64).reshape(-1)))
        return out if packed else rdm.unpack_rdm2(out, n)

    def rdm_info(self):
        """figures of the last rdm1 / rdm2 call: support size, rows, row chunks, real or complex form, workspace bytes, launch geometry
        of the Gram kernel, HIP-event times of the phases in microseconds"""
        out = (ctypes.c_int64 * 12)()
        self._ck(self._L.ovqe_rdm_info(self._h, out, 12))
        keys = ("nonzeros", "rows", "chunks", "real", "workspace_bytes", "gram_launches", "block_pairs", "row_slices",
                "list_us", "rows_us", "gram_us", "finish_us")
        return dict(zip(keys, [int(v) for v in out]))

    # -- Fubini-Study metric of the ansatz state (ovqe_metric_tensor, csrc/metric_host.inc) ----------------------------------------
    def metric_tensor(self, theta):
        """g[i, j] = Re(<T_i|T_j> - <T_i|psi><psi|T_j>), T_k = d psi / d theta_k, of the stored program at ``theta``: (K, K) float64,
        symmetric to the bit — the matrix of natural-gradient descent (``common_files.natural_gradient``)"""
        K = self._K
        theta = np.ascontiguousarray(theta, np.float64).reshape(-1)[:K]
        if theta.shape[0] != K:
            raise ValueError(f"expected {K} parameters")
        out = np.zeros((K, K), np.float64)
        self._ck(self._L.ovqe_metric_tensor(self._h, theta if K else np.zeros(1), K, out.reshape(-1) if K else np.zeros(1)))
        return out

    def metric_info(self):
        """figures of the last ``metric_tensor`` call: path (1 compact support, 2 streaming), parameters, amplitudes per tangent, bytes
        of the tangent store, launches of the tangent stage and of the Gram kernel, HIP-event times of the phases in microseconds, form of
        the tangent kernel (0 streaming, 1 compact with its tables staged in LDS, 2 compact with the tables read from global memory) and
        the dynamic LDS bytes of its launch"""
        out = (ctypes.c_int64 * 11)()
        self._ck(self._L.ovqe_metric_info(self._h, out, 11))
        keys = ("path", "K", "tangent_amplitudes", "store_bytes", "tangent_launches", "gram_launches", "tangents_us", "gram_us", "finish_us",
                "tangent_form", "tangent_lds_bytes")
        return dict(zip(keys, [int(v) for v in out]))

    # -- exact energy Hessian of the stored program (ovqe_energy_hessian, csrc/hessian_host.inc) -----------------------------------
    def energy_hessian(self, theta):
        """E(theta), the exact gradient and the exact Hessian d2E / dtheta_i dtheta_j of the stored program and Hamiltonian in one call
        -> (energy, grad[K], hess[K, K]); ``hess`` is symmetric to the bit, ``hessian_info()["asymmetry"]`` is max |M - M^T| of the raw
        rows (a built-in self-check) — the matrices of ``common_files.newton``"""
        K = self._K
        theta = np.ascontiguousarray(theta, np.float64).reshape(-1)[:K]
        if theta.shape[0] != K:
            raise ValueError(f"expected {K} parameters")
        e, asym = ctypes.c_double(), ctypes.c_double()
        grad = np.zeros(max(K, 1), np.float64)
        hess = np.zeros((K, K), np.float64)
        self._ck(self._L.ovqe_energy_hessian(self._h, theta if K else np.zeros(1), K, ctypes.byref(e), grad, hess.reshape(-1) if K else np.zeros(1),
                                             ctypes.byref(asym)))
        self._hessian_asymmetry = asym.value
        return e.value, grad[:K], hess

    def hessian_info(self):
        """figures of the last ``energy_hessian`` call: path (1 compact support, 2 streaming), parameters, amplitudes per vector, workspace
        bytes, launches, entries of the restricted Hamiltonian (path 1), HIP-event times of the phases in microseconds (path 1: the copy of
        theta to the device with the one launch, the copy back, 0; path 2: tangents and H images, the backward walk, the copy back), kernel form
        (0 streaming, 1 compact with its tables staged in LDS, 2 compact with the tables read from global memory), the dynamic LDS bytes of
        the launch, and ``asymmetry`` = max |M - M^T| of the raw rows"""
        out = (ctypes.c_int64 * 11)()
        self._ck(self._L.ovqe_hessian_info(self._h, out, 11))
        keys = ("path", "K", "amplitudes", "workspace_bytes", "launches", "entries", "phase0_us", "phase1_us", "phase2_us", "form", "lds_bytes")
        info = dict(zip(keys, [int(v) for v in out]))
        info["asymmetry"] = float(getattr(self, "_hessian_asymmetry", 0.0))
        return info

    # -- excited states by subspace expansion (ovqe_subspace_matrices, csrc/subspace_host.inc) ----------------------------------
    def _pack_pool_with_constants(self, ops):
        """CSR form of a list of operators, an operator's ``constant_coeff`` as a term on the identity string (x = z = 0); cached
        like the pool of ``pool_gradients`` (the pool is the same object from call to call)"""
        cache = getattr(self, "_subspace_cache", None)
        if cache is not None and cache[0] is ops and cache[1] == len(ops):
            return cache[2]
        offsets = np.zeros(len(ops) + 1, np.int64)
        xs, zs, cs = [], [], []
        for k, op in enumerate(ops):
            px, pz, pc = pack_terms(self.nbqbits, op.terms)
            const = complex(getattr(op, "constant_coeff", 0.0) or 0.0)
            if const != 0:
                px, pz, pc = np.append(px, np.uint64(0)), np.append(pz, np.uint64(0)), np.append(pc, const)
            xs.append(px)
            zs.append(pz)
            cs.append(pc)
            offsets[k + 1] = offsets[k] + px.shape[0]
        xs = np.concatenate(xs) if xs else np.zeros(0, np.uint64)
        zs = np.concatenate(zs) if zs else np.zeros(0, np.uint64)
        cs = np.concatenate(cs) if cs else np.zeros(0, np.complex128)
        if xs.shape[0] == 0:
            xs, zs, cs = np.zeros(1, np.uint64), np.zeros(1, np.uint64), np.zeros(1, np.complex128)
        packed = (offsets, np.ascontiguousarray(xs, np.uint64), np.ascontiguousarray(zs, np.uint64), np.ascontiguousarray(cs.real),
                  np.ascontiguousarray(cs.imag))
        self._subspace_cache = (ops, len(ops), packed)
        return packed

    def subspace_matrices(self, ops, hamiltonian=True, raw=False):
        """(H, S) of the subspace spanned by phi_j = O_j psi around the resident state, (m, m) complex128 each: S[i, j] = <phi_i|phi_j>
        (Hermitian to the bit), H[i, j] = <phi_i|H|phi_j> with the stored Hamiltonian and its constant, symmetrised as (G + G^H) / 2
        unless ``raw`` (then G = Phi^H (H Phi) as the device computed it).  ``hamiltonian=False``: only S, no Hamiltonian needed.
        ``ops``: operators with ``.terms`` (complex coefficients allowed) and optionally ``.constant_coeff``; solver: ``excited``"""
        m = len(ops)
        offsets, xs, zs, cre, cim = self._pack_pool_with_constants(ops)
        S = np.zeros((m, m), np.complex128)
        G = np.zeros((m, m), np.complex128) if hamiltonian else None
        self._ck(self._L.ovqe_subspace_matrices(self._h, m, offsets, xs, zs, cre, cim,
                                                G.view(np.float64).reshape(-1) if hamiltonian and m else None,
                                                S.view(np.float64).reshape(-1) if m else None))
        if not hamiltonian:
            return S
        return (G if raw else 0.5 * (G + G.conj().T)), S

    def subspace_info(self):
        """figures of the last ``subspace_matrices`` call: operators, rows of the store, dense form (no row lookup), store bytes,
        distinct x masks of the pool, x-groups of the Hamiltonian, launches of the expand / sigma / Gram stages, 64 x 64 block pairs
        computed, HIP-event times of the stages in microseconds, and the path the call took: row slices of the Gram launch and rows
        per slice, column blocks per lane of the sigma kernel that ran (1, 2 or 4; 0: none ran) and its column groups, workgroups in x
        of the sigma launch and workgroups of the expand launch"""
        out = (ctypes.c_int64 * 20)()
        self._ck(self._L.ovqe_subspace_info(self._h, out, 20))
        keys = ("m", "rows", "dense", "store_bytes", "distinct_x", "h_groups", "expand_launches", "sigma_launches", "gram_launches",
                "block_pairs", "rows_us", "expand_us", "sigma_us", "gram_us", "slices", "slice_rows", "sigma_blocks", "sigma_col_groups",
                "sigma_grid", "expand_grid")
        return dict(zip(keys, [int(v) for v in out]))

    # -- finite-shot measurement (ovqe_sample ..., csrc/measure_host.inc) --------------------------------------------------------
    def sample(self, n_shots, seed=0, stream=0, first_shot=0):
        """outcomes of shots ``first_shot .. first_shot + n_shots - 1`` drawn from |amplitude|^2 of the state in the buffer (which
        need not be normalised): uint64 basis indices, bit n-1-q = qubit q.  Shot s uses ``synth.shot_uniforms(seed, stream, s, 1)``."""
        out = np.zeros(int(n_shots), np.uint64)
        self._ck(self._L.ovqe_sample(self._h, int(n_shots), int(seed), int(stream), int(first_shot), out if n_shots else None))
        return out

    def measure_paulis(self, masks, coeffs, n_shots, xbasis=0, ybasis=0, seed=0, stream=0, first_shot=0, return_indices=False):
        """the same shots after the basis change (X on the index bits of ``xbasis``, Y on those of ``ybasis``), scored on diagonal
        terms: -> (term_sums int64 [T], (sum v, sum v^2)[, indices]) with v_s = sum_t coeffs[t] (-1)^popcount(b_s & masks[t])"""
        masks = np.ascontiguousarray(masks, np.uint64).reshape(-1)
        coeffs = np.ascontiguousarray(coeffs, np.float64).reshape(-1)
        if masks.shape != coeffs.shape:
            raise ValueError("masks and coeffs differ in length")
        T = masks.shape[0]
        tsum = np.zeros(T, np.int64)
        vsum = np.zeros(2, np.float64)
        idx = np.zeros(int(n_shots), np.uint64) if return_indices else None
        self._ck(self._L.ovqe_measure_paulis(self._h, int(xbasis), int(ybasis), int(n_shots), int(seed), int(stream), int(first_shot), T,
                                             masks if T else None, coeffs if T else None, tsum if T else None, vsum,
                                             idx if return_indices and n_shots else None))
        return (tsum, vsum, idx) if return_indices else (tsum, vsum)

    def measurement_groups(self):
        """the measurement plan of the stored Hamiltonian: (group of every stored term, -1 for identity terms; xbasis per group;
        ybasis per group) — qubit-wise commuting groups, first fit by |coeff| descending (include/ovqe_sv.h)"""
        G = ctypes.c_int64()
        cap = max(int(getattr(self, "_ham_terms", 0)), 1)
        got = np.full(cap, -1, np.int32)
        xb = np.zeros(cap, np.uint64)
        yb = np.zeros(cap, np.uint64)
        self._ck(self._L.ovqe_measure_groups(self._h, cap, got, xb, yb, ctypes.byref(G)))
        return got[:int(getattr(self, "_ham_terms", 0))], xb[:G.value], yb[:G.value]

    def energy_sampled(self, theta, n_shots, seed=0):
        """<H> of the stored program at ``theta`` from ``n_shots`` shots per measurement group -> (energy, standard error); leaves
        U(theta)|hf> in the state buffer like ``prepare_state``"""
        K = self._K
        theta = np.ascontiguousarray(theta, np.float64).reshape(-1)[:K]
        if theta.shape[0] != K:
            raise ValueError(f"expected {K} parameters")
        e, s = ctypes.c_double(), ctypes.c_double()
        self._ck(self._L.ovqe_energy_sampled(self._h, theta if K else None, K, int(n_shots), int(seed), ctypes.byref(e), ctypes.byref(s)))
        return e.value, s.value

    def measure_info(self):
        """figures of the last measuring call: groups, shots per group, scratch bytes, launches, HIP-event times of the phases in
        microseconds (summed over the groups), terms scored, streaming passes for rotated bits above the LDS tile"""
        out = (ctypes.c_int64 * 9)()
        self._ck(self._L.ovqe_measure_info(self._h, out, 9))
        keys = ("groups", "shots", "scratch_bytes", "launches", "basis_us", "scan_us", "draw_us", "terms", "high_passes")
        return dict(zip(keys, [int(v) for v in out]))

    def program_info(self):
        """shape of the compiled program: ops, rotations, literal gates, sweeps per evaluation, tiled sweeps,
        fused-kernel ops, support size (-1 = not analysed yet)"""
        out = (ctypes.c_int64 * 46)()
        self._ck(self._L.ovqe_program_info(self._h, out, 46))
        keys = ("ops", "rotations", "literal_gates", "sweeps", "tiled_sweeps", "fused_ops", "support",
                "h_tile_sweeps", "h_untiled_groups", "h_entries", "h_merged_terms", "h_pair_terms_per_tile",
                "real_stream", "sp_ops", "sp_pairs", "sp_h_entries",
                "sector_support", "sector_sweeps", "sector_pairs", "sector_h_sweeps", "sector_h_elements", "sector_bytes",
                "sector_circuit_us", "sector_expect_us", "sector_h_stream_bytes", "sector_fci_block",
                "sp_conflicts_discovery_order", "sp_conflicts", "sector_regular_slot_bits", "sector_free_bits",
                "sp_h_pieces", "sp_h_slots", "sp_h_reads_per_state",
                "sp_lds_row_reads", "sp_lds_row_writes", "sp_lds_h_reads",
                "sp_lds_row_reads_discovery_order", "sp_lds_row_writes_discovery_order",
                "sector_tile_bits", "sector_h_tile_bits", "sector_pair_slot_bits", "sector_max_tile", "sector_h_max_tile",
                "sector_h_max_dict", "sector_h_dict_entries", "sector_ordered_sweeps")
        return dict(zip(keys, [int(v) for v in out]))

    def rotation_program(self):
        """the stored program as its Pauli-rotation sequence (ovqe_get_rotation_program): a gate program in Clifford-frame form
        comes back with its conjugated strings.  -> (xs, zs, coeffs, phi0s, pidx) numpy arrays in execution order"""
        n = ctypes.c_int64()
        self._ck(self._L.ovqe_get_rotation_program(self._h, 0, None, None, None, None, None, ctypes.byref(n)))
        R = n.value
        xs, zs = np.empty(R, np.uint64), np.empty(R, np.uint64)
        cs, p0, pi = np.empty(R, np.float64), np.empty(R, np.float64), np.empty(R, np.int32)
        self._ck(self._L.ovqe_get_rotation_program(self._h, R, xs.ctypes.data, zs.ctypes.data, cs.ctypes.data, p0.ctypes.data,
                                                   pi.ctypes.data, ctypes.byref(n)))
        return xs, zs, cs, p0, pi

    # -- ADAPT ----------------------------------------------------------------------------------
    def pool_gradients(self, pool_ops, mode):
        """Gradient screen over ``pool_ops`` on the resident state, with the stored Hamiltonian.
        The packed form of the pool is cached (the pool is the same object in every ADAPT iteration)."""
        cache = getattr(self, "_pool_cache", None)
        if cache is not None and cache[0] is pool_ops and cache[1] == len(pool_ops):
            offsets, xs, zs, cs = cache[2]
        else:
            offsets = np.zeros(len(pool_ops) + 1, np.int64)
            xs, zs, cs = [], [], []
            for k, op in enumerate(pool_ops):
                px, pz, pc = pack_terms(self.nbqbits, op.terms)
                xs.append(px)
                zs.append(pz)
                cs.append(pc)
                offsets[k + 1] = offsets[k] + px.shape[0]
            xs = np.concatenate(xs) if xs else np.zeros(0, np.uint64)
            zs = np.concatenate(zs) if zs else np.zeros(0, np.uint64)
            cs = np.concatenate(cs) if cs else np.zeros(0, np.complex128)
            if xs.shape[0] == 0:
                xs, zs, cs = np.zeros(1, np.uint64), np.zeros(1, np.uint64), np.zeros(1, np.complex128)
            self._pool_cache = (pool_ops, len(pool_ops), (offsets, xs, zs, cs))
        out = np.zeros(len(pool_ops), np.float64)
        self._ck(self._L.ovqe_pool_gradients(self._h, len(pool_ops), offsets, xs, zs,
                                             np.ascontiguousarray(cs.real), np.ascontiguousarray(cs.imag),
                                             int(mode), out))
        return out

    def apply_exp_pauli_sum(self, operator, theta, prefactor=1.0):
        """psi <- exp(theta * prefactor * operator) psi, exact (no Trotter splitting)."""
        xs, zs, cs = pack_terms(self.nbqbits, operator.terms)
        cs = cs * prefactor
        if getattr(operator, "constant_coeff", 0.0):
            raise ValueError("apply_exp_pauli_sum: operator with a constant term")
        self._ck(self._L.ovqe_apply_exp_pauli_sum(self._h, xs.shape[0], xs, zs, np.ascontiguousarray(cs.real),
                                                  np.ascontiguousarray(cs.imag), float(theta)))

    def time_pauli_rotation(self, x, z, phi, warmup=3, reps=20):
        out = ctypes.c_double()
        self._ck(self._L.ovqe_time_pauli_rotation(self._h, int(x), int(z), float(phi), int(warmup), int(reps),
                                                  ctypes.byref(out)))
        return out.value


def device_count():
    c = ctypes.c_int()
    _lib.lib().ovqe_device_count(ctypes.byref(c))
    return c.value
