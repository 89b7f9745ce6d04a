/* ovqe_sv.h — C ABI of the MI355X-native statevector backend for OpenVQE's VQE / ADAPT-VQE
 * inner loop (libovqe_sv.so, gfx950 only).
 *
 * The reference (OpenVQE, pure Python) has no plugin ABI of its own: its hot path talks to the
 * third-party myQLM objects.  Each entry point below names the reference call
 * site(s) whose work it replaces ("ref:" = /root/reference/).
 *
 * Conventions
 *   - n-qubit state = 2^n complex<double> amplitudes (re,im interleaved, 16 B) resident in HBM.
 *   - reference qubit q  <->  basis-index bit (n-1-q)  (qubit 0 is the MSB:
 *     ref:openvqe/ucc_family/get_energy_qucc.py:40-45,
 *     ref:openvqe/common_files/molecule_factory_with_sparse.py:622-642,
 *     ref:openvqe/adapt/qubit_adapt_vqe.py:111-120).  ALL masks / bit numbers in this header are in
 *     basis-index bit space.
 *   - a Pauli string is two uint64 masks (x,z): I=(0,0) X=(1,0) Z=(0,1) Y=(1,1);
 *     P = i^{popcount(x&z)} X^x Z^z.
 *   - every function returns 0 on success or a negative OVQE_ERR_*; ovqe_last_error() gives text.
 *     No C++ exception crosses the ABI: every entry point is a function-try-block; std::bad_alloc -> OVQE_ERR_ALLOC,
 *     any other exception -> OVQE_ERR_INVALID with its what() in ovqe_last_error.  A handle is not thread-safe; distinct handles are
 *     independent.  Calls are synchronous unless stated (results are on the host on return).
 *   - host arrays are borrowed for the duration of the call only.
 *   - sharded states (multi-GPU): a handle may own one shard of 2^n_local amplitudes of a
 *     (n_local + n_global)-qubit state; shard s holds basis indices [s << n_local, (s+1) << n_local).
 *     Masks then span n_local+n_global bits; x bits must be local (the host layer makes them so by
 *     exchanging half shards, openvqe_amd/distributed.py), z bits may be global (rank-dependent sign).
 */
#ifndef OVQE_SV_H
#define OVQE_SV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OVQE_OK 0
#define OVQE_ERR_INVALID (-1)   /* bad argument */
#define OVQE_ERR_NO_DEVICE (-2) /* no usable gfx950 device */
#define OVQE_ERR_HIP (-3)       /* HIP runtime error (text in ovqe_last_error) */
#define OVQE_ERR_ALLOC (-4)     /* device/host allocation failed */
#define OVQE_ERR_STATE (-5)     /* call order: program / Hamiltonian not set */

/* gate opcodes of ovqe_set_gate_program / ovqe_apply_gate
 * (gate set of ref:openvqe/common_files/circuit.py:1 and ref:openvqe/ucc_family/get_energy_qucc.py:4;
 *  RX(a)=exp(-iaX/2), RY(a)=exp(-iaY/2), RZ(a)=diag(e^{-ia/2},e^{ia/2}), CNOT(control,target)) */
#define OVQE_GATE_X 0
#define OVQE_GATE_H 1
#define OVQE_GATE_RX 2
#define OVQE_GATE_RY 3
#define OVQE_GATE_RZ 4
#define OVQE_GATE_CNOT 5

/* pool-gradient modes */
#define OVQE_GRAD_FERMIONIC 0 /* g = 2 Re <sigma|A|psi>   ref:openvqe/adapt/fermionic_adapt_vqe.py:67-73 */
#define OVQE_GRAD_QUBIT 1     /* g = 2 |<sigma|P|psi>|    ref:openvqe/adapt/qubit_adapt_vqe.py:147-150 */

typedef struct ovqe_sv *ovqe_handle;

int ovqe_version(void);
/* text of the last error on this handle (h may be NULL: last error of a failed create) */
const char *ovqe_last_error(ovqe_handle h);
int ovqe_device_count(int *count);

/* ---- lifecycle.  Replaces the per-submit state allocation of qat.qpus.get_default_qpu().submit
 * (ref:openvqe/ucc_family/get_energy_ucc.py:38-48): the library owns the device buffers.
 * 1 <= n_qubits (n_local) <= 33 per device (128 GiB state); larger registers are sharded. */
int ovqe_create(int n_qubits, int device, ovqe_handle *out);
/* one shard of a distributed state: n_local local bits, n_global rank bits, this shard's index */
int ovqe_create_shard(int n_local, int n_global, uint64_t shard_index, int device, ovqe_handle *out);
/* a handle whose state IS the caller's device buffer of 2^n_qubits amplitudes (16 bytes each) from the start: nothing of that
 * size is allocated (ovqe_create + ovqe_adopt_state would allocate a state and drop it).  The sharded register contracts CHUNKS of
 * partner shards through such views (the chunk contractions of <psi|H|psi> / sigma = H psi over a partitioned register, the
 * multi-device form of ref:openvqe/adapt/fermionic_adapt_vqe.py:114 and get_energy_ucc.py:47-48); the buffer must outlive the handle. */
int ovqe_create_view(int n_qubits, int device, void *dev_ptr, ovqe_handle *out);
int ovqe_destroy(ovqe_handle h);
/* run this handle's kernels on a caller-owned hipStream_t (NULL = default stream) */
int ovqe_set_stream(ovqe_handle h, void *hip_stream);
/* Options.  None of them changes a result beyond rounding (tests/test_gpu_tile.py, test_gpu_kernels.py, test_gpu_sector.py compare the
 * settings with one another and with the oracle); unknown names return OVQE_ERR_INVALID.  Three groups:
 *
 * (A) WHICH PATH RUNS — what a caller may reasonably set
 *   "force_path"      0 automatic (default), 1 fused small-register kernel, 2 streaming kernels, 3 support-compacted kernel
 *   "clifford_frame"  read by the NEXT ovqe_set_gate_program.  1 (default): a gate list whose Clifford part (X, H, CNOT, quarter-turn
 *                     rotations) multiplies to the identity runs as the algebraically identical sequence of Pauli rotations with
 *                     conjugated strings; when it does NOT close (interleaved CNOT ladders, stray gates) that rotation sequence runs
 *                     too, energies / gradients then use the stored Hamiltonian conjugated by the net Clifford operator
 *                     (<C phi|H|C phi> = <phi|C^+ H C|phi>, every term stays one Pauli string) and ovqe_prepare_state applies the
 *                     Clifford gates behind the rotations.  0: execute the literal list; 2: frame form always, Clifford part appended
 *                     literally; 3: frame form only when the frame closes
 *   "real_mode" / "real_stream" (1)  a program whose rotation strings all have an odd number of Y (every UCC / ADAPT generator, the
 *                     QUCCSD templates in frame form) keeps the amplitudes real: 8-byte amplitudes in the fused kernel / 2^n doubles in
 *                     streaming energies (n >= 15): half the bytes per sweep; ovqe_prepare_state always delivers the complex state
 *   "table_fusion" (1) commuting same-x runs become single sparse pair rotations in the fused kernel
 *   "clifford_phase_host" (1)  the global phase that the Clifford part of a closed gate list gives |hf> (ovqe_prepare_state reproduces the
 *                     literal circuit's phase) from a sparse simulation on the host; 0 or more than 4096 basis states: the gates run on
 *                     the device
 *   "sparse" (1)      support-compacted kernel when the program's reachable support fits one workgroup's LDS
 *   "compact" (1)     compact cover: from the second evaluation of a (program, Hamiltonian) pair, <H> of a real-amplitude streaming
 *                     energy runs over a compact copy of the state's support
 *   "sector" (1)      sector path: from the second energy evaluation (the first gradient call; the first evaluation for programs of at most
 *                     2048 rotations) a real-amplitude program whose states occupy at most 1/"sector_sparsity" (4) of
 *                     the register runs entirely on that support: circuit over compact tiles, <H> from the Hamiltonian materialised on
 *                     the support; tables in device memory up to "sector_max_gb" (128; and 60 % of the free memory) — beyond it <H> goes
 *                     through the compact cover; "sector_min_qubits" (18); "sector_h" 0: never materialise <H>.  When an evaluation meets
 *                     a non-zero amplitude whose partner is outside the probed support it is redone by the dense kernels and the tables are
 *                     rebuilt once from a probe with one angle per rotation.  The state buffer holds unspecified data after an energy
 *                     evaluation on this path.
 *   "sector_regular" (1)  supports that are the full coset of the program's Z2 symmetries (the spin-parity quarter that the reference's
 *                     QUCCSD templates populate): circuit sweeps — and with "sector_reg_adjoint" (1) the backward sweeps of
 *                     ovqe_energy_gradient — from bit arithmetic, no pair-word tables for supports of 2^20 amplitudes and more; 0: pair
 *                     words; 3: without the slot orders that make the gathers between sweeps run in runs (measurement)
 *   "sector_batch" (1) ovqe_energy_batch / _device run whole batches per pass of the sector tables
 *   "poll_result" (1)  the host of a lone evaluation — or of a batch of at most 256 on the fused kernels (a finite-difference gradient) —
 *                     watches the mapped slots its kernels write instead of waiting for the stream's completion signal (6 us per call;
 *                     evaluations of the sector tables that took less than 2 ms the time before, the fused kernels always); nothing
 *                     within 5 ms: the stream is synchronised after all
 *   "sector_fused_reduce" (1)  the final reduction of a lone evaluation on the sector tables writes energy and orphan flag into mapped
 *                     host memory; 0: reduction launch + two copies
 *   "screen_sparse" (16) / "screen_sector" (1) / "screen_sector_min" (1024)  ADAPT screens: bilinear forms summed over
 *                     the listed non-zero amplitudes of psi while they are at most 1/value of the register (0: never); sigma = H psi from the
 *                     materialised Hamiltonian of psi's symmetry sector once psi lists that many amplitudes; pattern tables for the pool's
 *                     same-x runs (see ovqe_pool_gradients, ovqe_last_support); ovqe_apply_exp_pauli_sum runs its Taylor steps over the
 *                     closure of the support under the operator's x-groups within the same bound (bit-identical amplitudes)
 *   "lanczos_keep_gb" (160) ovqe_ground_state keeps its Lanczos vectors in HBM up to this many GB (and 60 % of the free memory): one pass of
 *                     the recurrence gives the Ritz vector; 0 or vectors that do not fit: the recurrence runs twice
 *   "rdm_workspace_mb" (1024)  ovqe_rdm materialises its rows in chunks of at most this many MB of device memory (at least one staging
 *                     tile of 16 or 32 rows); the buffer is allocated at the first call that needs it and kept on the handle
 *   "metric_workspace_mb" (0)  cap of the tangent store of ovqe_metric_tensor in MB; 0: 60 % of the free device memory.  A store beyond
 *                     the cap is refused with OVQE_ERR_ALLOC; the buffer is allocated at the first call and kept on the handle
 *   "subspace_workspace_mb" (0)  cap of the store of ovqe_subspace_matrices (expansion vectors and their H images) in MB; 0: 60 % of the
 *                     free device memory.  A store beyond the cap is refused with OVQE_ERR_ALLOC; allocated at the first call, kept on the handle
 *
 *   "real_state" (0)  the state buffer holds 2^n_local DOUBLES (8 bytes per amplitude: a shard of the partitioned register while its
 *                     amplitudes are real).  BUFFER-SIZE CONTRACT: while it is set, the state and every shard-sized operand of
 *                     ovqe_init_basis, ovqe_randomize, ovqe_norm2, ovqe_apply_pauli_rotations (odd-Y strings only), ovqe_shard_pack / _unpack,
 *                     ovqe_xsum_expect_*, ovqe_xsum_apply_* (out_dev; ket_chunk = 2^chunk_bits doubles) and ovqe_vec_* is 2^n_local
 *                     doubles; the caller sets it together with ovqe_adopt_state of a buffer of that size.  Every other entry
 *                     point keeps reading 16-byte amplitudes: clear the option and widen the buffer before calling one.
 *
 * (B) GEOMETRY — defaults are the measured optimum on MI355X
 *   streaming path: "tile_bits" (-1 automatic: 12 for n >= 25, else 11; 0 = one sweep per op), "tile_low" (4), "apply_min_tiles" (256),
 *                     "index_streams"; "adjoint_tile_bits" (-1 automatic: 12 for n >= 25, else 11; 0 = one backward pass per run) of ovqe_adjoint_rotations
 *                     "grad_batch_waves" (0 automatic; 1, 2, 4, 8: waves per workgroup of ovqe_energy_gradient_batch's kernel, other values read
 *                     as 0), "grad_batch_workgroups" (0 automatic; otherwise a cap on its grid)
 *   fused / support-compacted kernels: "small_max_qubits", "small_batch_max_qubits", "sparse_grad" (1: all derivatives of a register of at most
 *                     16 qubits in one fused launch on the compact support; 0: the streaming adjoint pass), "sparse_renumber" (1)
 *   sector path: "sector_bits" / "sector_h_bits" (index bits per circuit / <H> tile, 0 automatic), "sector_tile_cap" (6500 amplitudes per
 *                     circuit tile so that gradients fit; up to 14000 for energies only), "sector_threads" (0 automatic, 64, 256, 512,
 *                     1024), "sector_adjoint" (backward sweeps of the gradient: 3 on the per-wave streams where a sweep has them, 2 on the 64-bit
 *                     pair tables, 1 first form), "sector_dict" (1: dictionary-coded matrix elements, dictionary from a sample of the
 *                     stream first; 2: from all values; 3: from a sample too thin to be complete — the fall-back, tests; 0: explicit values),
 *                     "sector_reg_threads" (256; 128, 512, 1024), "sector_reg_pairs" (1: blocks of two three-bit ops), "sector_reg_runs"
 *                     (1: runs of ops whose waves stay inside their own slots run without barriers), "sector_pairs_form" (2: pair-table
 *                     builder with the ops staged in LDS; 1: first form).  Combinations the second sweep form has no kernel for fall back to
 *                     the first form / to one evaluation at a time.
 *   "sector_profile"  HIP-event times of the two halves of a sector evaluation in ovqe_program_info
 *
 * (C) MEASUREMENT AND TESTS — accepted ONLY by the testing build of this same source (-DOVQE_TESTING: libovqe_sv_testing.so, loaded by
 *   tests/test_gpu_abi.py and, through OVQE_LIB=testing, by the scripts under tools/); the product library answers OVQE_ERR_INVALID
 *   "unknown option" and runs every one of them at its default:
 *   "fault_inject" (1: the next term-list build throws std::bad_alloc: the exception barrier's test), "sector_debug" (2: say on stderr why a
 *   program was left to the dense kernels; 4: wall time of the build's phases), "sector_sweep_dbg" / "sector_h_dbg" / "sparse_dbg" (kernels
 *   truncated after a given phase), and the launch geometries and superseded forms kept for comparison: "sparse_rows", "sparse_wg",
 *   "sparse_shared" (0: large batches of the rows form on one wave per pair of evaluations instead of the workgroup geometry, 2: that geometry below its batch threshold too),
 *   "sparse_pack" (0: the restricted Hamiltonian counts as one that does not pack into the workgroup geometry's owner pieces: the selection's fall-back), "sparse_spw", "sector_sweep" (circuit sweeps on an irregular support: 3 pair words in per-wave streams with barriers at
 *   run boundaries only — built on top of the tables of 2 —, 2 64-bit pair words in registers with a barrier per round, 1 first form; 2 on a
 *   handle built under 3 runs the second form on the same tables; 4: the streams for the states of a batch too — the product gives
 *   batches the second form: their workgroups hide each other's barriers and the streams gain them nothing), "sector_stream_waves" (0: waves that share a tile's rows from the pairs per
 *   op of the sweep's largest tile; 1, 2, 4, 8, 16), "sector_stream_arrange" (1: the lanes of a row chosen for the LDS banks), "sector_h_pack" (1: <H> sweeps with at most 1023
 *   magnitudes keep their coded words as 24-bit elements), "sector_eager_rots", "tile_flat" (tiled <H>: entries of one
 *   or two merged terms as per-lane items 1 / per-wave entries 0 / items for real states only 2, the default), "expect_dense" (1: the
 *   first sweep of a tiled <H> of a complex register of 25+ qubits counts its sparse tiles; none: the other sweeps run without the
 *   sparse path's LDS, two workgroups per CU) */
int ovqe_set_option(ovqe_handle h, const char *name, int64_t value);
/* device pointer to the 2^n_local amplitudes (for RCCL exchange by the host layer).  The caller may write them between calls: from
 * here on the handle keeps nothing it learnt about the state from one call to the next (the support list that a chain of
 * ovqe_apply_exp_pauli_sum calls otherwise carries over is listed afresh per call) */
int ovqe_state_ptr(ovqe_handle h, void **dev_ptr);
/* use caller-owned device memory (e.g. a torch tensor) of 2^n_local*16 bytes as the state buffer */
int ovqe_adopt_state(ovqe_handle h, void *dev_ptr);

/* ---- state set-up / read-back */
/* |index> (global index).  HF reference state: X on qubit q iff bit (n-1-q) of hf_init is set
 * (ref:openvqe/ucc_family/get_energy_ucc.py:43 `init`, get_energy_qucc.py:40-45;
 *  ref:openvqe/adapt/fermionic_adapt_vqe.py:183-213 prepare_hf_state) */
int ovqe_init_basis(ovqe_handle h, uint64_t index);
int ovqe_set_state(ovqe_handle h, const double *amps_re_im);       /* 2*2^n_local doubles */

/* The state as the list of its non-zero amplitudes, ascending index (what iterating a myQLM Result of a state-vector job yields,
 * ref:openvqe/adapt/fermionic_adapt_vqe.py:309-328 get_statevector): *count = number of non-zero amplitudes; indices[0..*count) and
 * amps[0..2 * *count) (re, im) are filled when *count <= capacity (else only the count is returned: call again, or ovqe_get_state).
 * *count = -1 on registers below 12 qubits and on shards of a distributed register (use ovqe_get_state there). */
int ovqe_get_support(ovqe_handle h, int64_t capacity, uint64_t *indices, double *amps, int64_t *count);
/* full-statevector read-back (ref:openvqe/adapt/fermionic_adapt_vqe.py:309-328 get_statevector) */
int ovqe_get_state(ovqe_handle h, double *amps_re_im);
int ovqe_get_amplitudes(ovqe_handle h, int64_t count, const uint64_t *local_indices, double *amps_re_im);
/* deterministic synthetic state: amp(i) = scale * (u1(i), u2(i)), u in [-1,1) from a counter-based
 * integer hash of (seed, global index) (bit-reproducible on the host, see openvqe_amd/synth.py);
 * scale normalises the FULL state when norm2_total > 0 is given, else this shard alone.
 * Returns the scale used.  Under option "real_state" the 2^n_local doubles take the REAL parts of that fill (amp(i) = scale * u1(i)
 * at the same global index: independent of the partition) and the shard's own norm counts those alone. */
int ovqe_randomize(ovqe_handle h, uint64_t seed, double norm2_total, double *scale_out);
int ovqe_norm2(ovqe_handle h, double *out); /* sum |a_i|^2 over this shard */

/* ---- unit operations on the resident state (large-n, HBM-bound path) */
/* psi <- exp(-i phi P) psi : the unit of work of build_ucc_ansatz([op], init, n_steps=1)([theta])
 * (third-party; call sites ref:openvqe/ucc_family/get_energy_ucc.py:44,86,
 *  ref:openvqe/adapt/fermionic_adapt_vqe.py:158,302, ref:openvqe/adapt/qubit_adapt_vqe.py:181,303) */
int ovqe_apply_pauli_rotation(ovqe_handle h, uint64_t x, uint64_t z, double phi);
/* R rotations in order; consecutive rotations sharing an x mask are fused into one sweep */
int ovqe_apply_pauli_rotations(ovqe_handle h, int64_t R, const uint64_t *x, const uint64_t *z, const double *phi);
/* one literal gate (ref:openvqe/common_files/circuit.py:13-93 templates); b0 = target/control bit, b1 = CNOT target */
int ovqe_apply_gate(ovqe_handle h, int opcode, int b0, int b1, double angle);
/* Re sum_t coeff[t] <psi|P_t|psi> + constant  (shard-local partial sum when sharded):
 * circ.to_job(job_type="OBS", observable=H) + qpu.submit(job).value
 * (ref:openvqe/ucc_family/get_energy_ucc.py:46-48, get_energy_qucc.py:52-54,
 *  ref:openvqe/adapt/fermionic_adapt_vqe.py:161,237, ref:openvqe/adapt/qubit_adapt_vqe.py:209,267,306) */
int ovqe_expectation(ovqe_handle h, int64_t T, const uint64_t *x, const uint64_t *z, const double *coeff,
                     double constant, double *out);
/* sum_t coeff[t] <bra|P_t|ket> with explicit device buffers of 2^n_local amplitudes each
 * (bra/ket NULL = this handle's state).  Used for global-x Hamiltonian terms across shards. */
int ovqe_bilinear(ovqe_handle h, const void *bra_dev, const void *ket_dev, int64_t T, const uint64_t *x,
                  const uint64_t *z, const double *coeff_re, const double *coeff_im, double *out_re_im);

/* out (+)= sum_t (coeff_re + i coeff_im)[t] P_t ket, explicit device buffers of 2^n_local amplitudes (ket NULL = this
 * handle's state; out != ket).  x masks may carry ONE global (rank) part when ket is the partner shard with that rank
 * difference: sigma = H psi of a sharded register, assembled group by group by the host layer
 * (ref:openvqe/adapt/fermionic_adapt_vqe.py:114 `sig = hamiltonian_sparse.dot(curr_state)`). */
int ovqe_apply_pauli_sum(ovqe_handle h, const void *ket_dev, void *out_dev, int64_t T, const uint64_t *x, const uint64_t *z,
                         const double *coeff_re, const double *coeff_im, int accumulate);
/* out[k] = sum_{j in [off[k], off[k+1])} c_j <bra|P_j|ket> (complex, interleaved re/im) for n_ops operators in one launch;
 * bra / ket as in ovqe_bilinear; all x masks of one call share their global part (the pool gradients of a sharded
 * register: bra = sigma shard, ket = psi shard of the partner; ref:openvqe/adapt/fermionic_adapt_vqe.py:67-73). */
int ovqe_bilinear_batch(ovqe_handle h, const void *bra_dev, const void *ket_dev, int64_t n_ops, const int64_t *offsets,
                        const uint64_t *x, const uint64_t *z, const double *coeff_re, const double *coeff_im,
                        double *out_re_im);

/* ---- Pauli sums planned once for a shard of the partitioned register ("group terms by x_g ... exchange
 * (read-only) + local partial sums"; the observable of ref:openvqe/ucc_family/get_energy_ucc.py:46-48 and the sigma = H psi of
 * ref:openvqe/adapt/fermionic_adapt_vqe.py:114 on a register that no single device holds).  Masks live in the PHYSICAL index-bit space
 * of the whole register (n_local + n_global bits).  d = x >> n_local names the shard (this shard's index ^ d) a term reads its ket
 * amplitudes from; the host layer (openvqe_amd/distributed.py) receives that shard in chunks of 2^chunk_bits amplitudes and hands
 * every chunk to the calls below.  The plan — d = 0 terms as a tile cover of the shard, the others as LDS-tiled passes over
 * (chunk, own shard) pairs, csrc/sv_cross.hpp — is made once; an evaluation uploads nothing.  *_remote calls only enqueue work on the
 * handle's stream (ovqe_set_stream: order them behind the transfer of the chunk); expect_local / expect_finish synchronise. */
int ovqe_xsum_create(ovqe_handle h, int64_t T, const uint64_t *x, const uint64_t *z, const double *coeff_re, const double *coeff_im,
                     int chunk_bits, int32_t *id);
int ovqe_xsum_destroy(ovqe_handle h, int32_t id);
/* the rank differences d != 0 the sum has terms for (ascending) and the passes one chunk of each costs; *count = how many */
int ovqe_xsum_partners(ovqe_handle h, int32_t id, int64_t capacity, uint64_t *d, int64_t *passes, int64_t *count);
/* info[0..10): local x-groups, local terms, local tile sweeps (0 until the first evaluation), local groups outside the cover,
 * partners, remote x-groups, remote terms, remote passes per chunk summed over the partners, tile bits of the passes, 1 when the
 * chunks are too small to tile (streaming kernel) */
int ovqe_xsum_info(ovqe_handle h, int32_t id, int64_t *info, int count);
/* Re <shard| H_0 |shard> of the d = 0 terms (real coefficients only) */
int ovqe_xsum_expect_local(ovqe_handle h, int32_t id, double *out);
/* accumulate <shard| H_d |ket> for chunk `chunk` of the shard of (this shard's index ^ d): ket_chunk = 2^chunk_bits amplitudes on
 * this device */
int ovqe_xsum_expect_remote(ovqe_handle h, int32_t id, uint64_t d, uint64_t chunk, const void *ket_chunk);
/* the accumulated remote contractions (re, im) since the last finish; resets the accumulator */
int ovqe_xsum_expect_finish(ovqe_handle h, int32_t id, double *out_re_im);
/* out = ident * psi + H_0 psi on this shard's state (out: 2^n_local amplitudes, != the state).  Under option "real_state" out holds
 * 2^n_local doubles and must not overlap the state; a sum that does not map real vectors to real vectors (a string with an odd
 * number of Y, a coefficient with an imaginary part) is refused with OVQE_ERR_STATE, here and in ovqe_xsum_apply_remote */
int ovqe_xsum_apply_local(ovqe_handle h, int32_t id, void *out_dev, double ident);
/* out += H_d ket for one received chunk (out: the 2^n_local-amplitude buffer being accumulated; under "real_state" ket_chunk is
 * 2^chunk_bits doubles and out 2^n_local doubles) */
int ovqe_xsum_apply_remote(ovqe_handle h, int32_t id, uint64_t d, uint64_t chunk, const void *ket_chunk, void *out_dev);

/* ---- The ADAPT pool screen planned once for a shard of the partitioned register: v_k = sum_t c_t <sigma| P_t |psi> for every pool
 * operator k (g_k = 2 Re v_k, ref:openvqe/adapt/fermionic_adapt_vqe.py:41-122; g_k = 2 |v_k|, ref:openvqe/adapt/qubit_adapt_vqe.py:126-150)
 * with sigma = H psi resident on this rank (ovqe_xsum_apply_*) and psi arriving chunk by chunk, as for the sums above.  Terms in CSR
 * form (offsets[0..n_ops], never decreasing), masks in the PHYSICAL index-bit space of the whole register.  The plan — per rank
 * difference d = x >> n_local a greedy cover of the distinct local x masks by LDS-tiled passes that evaluate EVERY operator of the
 * pass from one staging of the ket tile (csrc/sv_pool_host.hpp, csrc/sv_pool.hpp; chunks below 2^10 complex / 2^11 real amplitudes
 * stream) — is made once per (pool, permutation, chunk bits); a screen uploads nothing.  Partial sums: 512 rows x n_ops x 16 bytes
 * whatever the shard, reduced in a fixed order (results are bit-identical from run to run).  Under option "real_state" bra and ket
 * are doubles and both parts of v_k are kept: real folded coefficients c i^ny give Re v_k, imaginary ones Im v_k. */
int ovqe_xpool_create(ovqe_handle h, int64_t n_ops, const int64_t *offsets, const uint64_t *x, const uint64_t *z, const double *coeff_re,
                      const double *coeff_im, int chunk_bits, int32_t *id);
int ovqe_xpool_destroy(ovqe_handle h, int32_t id);
/* the rank differences d != 0 the pool has entries for (ascending) and the passes one chunk of each costs; *count = how many */
int ovqe_xpool_partners(ovqe_handle h, int32_t id, int64_t capacity, uint64_t *d, int64_t *passes, int64_t *count);
/* info[0..9): operators, (operator, local x) entries, distinct local x masks summed over the rank differences, partners, passes per
 * chunk summed over the partners, passes of the d = 0 entries over the shard, tile bits of the passes, 1 when a chunk is too small
 * to tile (streaming kernel), bytes of the partial sums */
int ovqe_xpool_info(ovqe_handle h, int32_t id, int64_t *info, int count);
/* accumulate the d = 0 entries: bra = bra_dev (the sigma shard: 2^n_local amplitudes, not overlapping the state), ket = the handle's
 * state (ref:openvqe/adapt/fermionic_adapt_vqe.py:67-73).  Only enqueues on the handle's stream. */
int ovqe_xpool_local(ovqe_handle h, int32_t id, const void *bra_dev);
/* accumulate the entries of rank difference d for chunk `chunk` of the shard of (this shard's index ^ d): ket_chunk = 2^chunk_bits
 * amplitudes on this device.  Only enqueues on the handle's stream; afterwards ovqe_last_support(4 / 5) = the passes over the chunk
 * and the bytes they move by construction (32 B, or 16 B under "real_state", per amplitude and pass). */
int ovqe_xpool_remote(ovqe_handle h, int32_t id, uint64_t d, uint64_t chunk, const void *ket_chunk, const void *bra_dev);
/* v_k as (re, im) pairs, 2 * n_ops doubles (ref:openvqe/adapt/qubit_adapt_vqe.py:147-150 takes |v_k|): the accumulated local and
 * remote contractions since the last finish; resets the accumulators and synchronises */
int ovqe_xpool_finish(ovqe_handle h, int32_t id, double *out_re_im);

/* ---- Lanczos vector operations on caller-held device buffers of the handle's storage (2^n_local amplitudes of 16 bytes, or 2^n_local
 * doubles under option "real_state"): the steps of ovqe_ground_state for a host layer that runs the recurrence over a partitioned
 * register (openvqe_amd/distributed.py ground_state; ref:openvqe/adapt/fermionic_adapt_vqe.py:419 takes the same eigenpair from a
 * sparse matrix on one host).  Each returns the partial of THIS shard — the library never communicates.  dot and lanczos_update
 * synchronise the handle's stream; scale and axpy only enqueue on it. */
/* sum_i conj(a_i) b_i -> (re, im); im = 0 under "real_state" */
int ovqe_vec_dot(ovqe_handle h, const void *a_dev, const void *b_dev, double *out_re_im);
/* w <- w - alpha v - beta v_prev (v_prev may be NULL), *norm2_out = sum_i |w_i|^2 of the result */
int ovqe_vec_lanczos_update(ovqe_handle h, void *w_dev, const void *v_dev, const void *vprev_dev, double alpha, double beta,
                            double *norm2_out);
/* v <- s v */
int ovqe_vec_scale(ovqe_handle h, void *v_dev, double s);
/* y <- y + s x, or y <- s x when overwrite != 0 */
int ovqe_vec_axpy(ovqe_handle h, void *y_dev, const void *x_dev, double s, int overwrite);

/* ---- k-bit shard exchange of a partitioned register (openvqe_amd/distributed.py: k global index bits traded for k local ones in one
 * all-to-all among the 2^k ranks of a sub-cube; the many-device form of the state that qpu.submit keeps on one host,
 * ref:openvqe/ucc_family/get_energy_ucc.py:46-48).  local_bit_mask: the k = 1..6 local physical bits L being exchanged (anywhere below
 * n_local); block: a k-bit value b.  The block's 2^(n_local - k) amplitudes in ascending order: position j sits at
 * deposit(j, ~L) | deposit(b, L) in the shard.  pack: dst[j - first] = state[that index] for j in [first, first + count); unpack is the
 * inverse scatter (amplitudes outside the range untouched).  Elements are what the handle stores: 16-byte complex, or 8-byte doubles
 * under option "real_state"; with complex storage and real_parts_only != 0 the stream holds the real parts only (8 bytes each) and
 * unpack writes exact zero imaginary parts.  Both only enqueue on the handle's stream (ovqe_set_stream): no synchronisation, no
 * allocation.  The buffer is device memory aligned to its elements. */
int ovqe_shard_pack(ovqe_handle h, uint64_t local_bit_mask, uint64_t block, int64_t first, int64_t count, void *dst,
                    int real_parts_only);
int ovqe_shard_unpack(ovqe_handle h, uint64_t local_bit_mask, uint64_t block, int64_t first, int64_t count, const void *src,
                      int real_parts_only);

/* ---- compiled evaluation: E(theta) of a whole ansatz circuit */
/* observable H = constant + sum_t coeff[t] P_t (real coefficients; ref:...get_energy_ucc.py:47) */
int ovqe_set_hamiltonian(ovqe_handle h, int64_t T, const uint64_t *x, const uint64_t *z, const double *coeff,
                         double constant);
/* Pauli-rotation program on |hf_index>: rotation r is exp(-i (coeff[r]*theta[pidx[r]] + phi0[r]) P_r)
 * (pidx[r] < 0: constant angle phi0[r]; phi0 may be NULL); K = number of parameters.
 * This is the flattened form of the loop ref:openvqe/ucc_family/get_energy_ucc.py:42-45
 * (and fermionic_adapt_vqe.py:156-159, qubit_adapt_vqe.py:301-304). */
int ovqe_set_program(ovqe_handle h, int64_t R, const uint64_t *x, const uint64_t *z, const double *coeff,
                     const double *phi0, const int32_t *pidx, int32_t K, uint64_t hf_index);
/* literal gate program on |hf_index>: gate g has angle ascale[g]*theta[pidx[g]] + aconst[g]
 * (ref:openvqe/ucc_family/get_energy_qucc.py:37-51 + circuit.py:95-106 efficient_fermionic_ansatz).
 * With option "clifford_frame" != 0 the call OVERWRITES the resident state buffer (the Clifford part of the list is
 * executed once on |hf_index> to read its global phase); on any error the handle is left with NO program set. */
int ovqe_set_gate_program(ovqe_handle h, int64_t G, const int32_t *opcode, const int32_t *b0, const int32_t *b1,
                          const double *ascale, const double *aconst, const int32_t *pidx, int32_t K,
                          uint64_t hf_index);
/* E(theta): one call == one ucc_action / action_quccsd evaluation
 * (ref:openvqe/ucc_family/get_energy_ucc.py:8-50, get_energy_qucc.py:11-56).  The content of the state buffer after an
 * energy call is unspecified (the fused kernels never touch it, the streaming path may hold real amplitudes there):
 * use ovqe_prepare_state to obtain U(theta)|hf>. */
int ovqe_energy(ovqe_handle h, const double *theta, int32_t K, double *energy);
/* B parameter vectors (row-major B x K) in one launch — one finite-difference gradient of
 * scipy.optimize.minimize(jac=None) (ref:openvqe/ucc_family/get_energy_ucc.py:158-175) is B = K+1 */
int ovqe_energy_batch(ovqe_handle h, int64_t B, const double *theta, int32_t K, double *energies);
/* same with theta (B x K doubles) and energies (B doubles) RESIDENT ON THE DEVICE (e.g. theta batches produced on the GPU, or
 * uploaded once and re-used): nothing crosses PCIe on the fused kernels (n <= 16) and on the batched sector evaluations (real-amplitude
 * programs with sector tables: whole batches per pass of the tables); any other program is served through the host, one
 * evaluation at a time (B x K doubles down, B energies up) */
int ovqe_energy_batch_device(ovqe_handle h, int64_t B, const void *theta_dev, int32_t K, void *energies_dev);
/* run the program and leave U(theta)|hf> in the handle's state buffer
 * (prepare_state_ansatz + get_statevector, ref:openvqe/adapt/fermionic_adapt_vqe.py:273-328) */
int ovqe_prepare_state(ovqe_handle h, const double *theta, int32_t K);

/* ---- ADAPT gradient screen on the resident state psi (uses the stored Hamiltonian):
 * sigma = H psi once, then for pool operator k = sum_{j in [off[k],off[k+1])} c_j P_j
 *   mode FERMIONIC: g_k = 2 Re sum_j c_j <sigma|P_j|psi>   (c complex; A_k anti-Hermitian)
 *   mode QUBIT    : g_k = 2 | sum_j c_j <sigma|P_j|psi> |
 * (ref:openvqe/adapt/fermionic_adapt_vqe.py:41-122, ref:openvqe/adapt/qubit_adapt_vqe.py:126-150,462-471) */
int ovqe_pool_gradients(ovqe_handle h, int64_t n_ops, const int64_t *offsets, const uint64_t *x, const uint64_t *z,
                        const double *coeff_re, const double *coeff_im, int mode, double *grads);
/* psi <- exp(theta * A) psi with A = sum_t (coeff_re+i coeff_im)[t] P_t, exact (scaled Taylor series),
 * the state evolution of the gradient screens
 * (ref:openvqe/adapt/fermionic_adapt_vqe.py:12-38 expm_multiply; qubit_adapt_vqe.py:20-55 expm(-i theta P)) */
int ovqe_apply_exp_pauli_sum(ovqe_handle h, int64_t T, const uint64_t *x, const uint64_t *z, const double *coeff_re,
                             const double *coeff_im, double theta);

/* ---- E(theta) and its EXACT gradient dE/dtheta[K] by the adjoint (reverse-mode) method: psi = U(theta)|hf>,
 * lambda = H psi, then one backward pass over the program that un-applies every rotation from both states and reads
 * dE/dtheta_p = sum_{r: pidx_r = p} 2 c_r Im <lambda_r|P_r|psi_r> on the way — about three circuit executions for
 * ALL K derivatives, where the reference's BFGS (jac=None, ref:openvqe/ucc_family/get_energy_ucc.py:158-175) spends K+1
 * evaluations on forward differences (opt-in, because exact derivatives change the
 * optimiser's iterates at the 1e-8 level).  Streaming kernels, any n; the state buffer is left in |hf>.  A real-amplitude
 * program with sector tables (option "sector"; built by the first gradient call when they do not exist yet) runs the whole
 * pass on them: forward circuit,
 * lambda = H psi from the materialised Hamiltonian, backward sweeps over the pair lists. */
int ovqe_energy_gradient(ovqe_handle h, const double *theta, int32_t K, double *energy, double *grad);

/* ---- backward step of the adjoint method on a (psi, lambda) pair the CALLER holds: what a partitioned register runs between
 * its shard exchanges (openvqe_amd/distributed.py: program_energy_gradient), so that the exact Jacobian of
 * ref:openvqe/ucc_family/get_energy_ucc.py:42-50 (the energy the optimiser differentiates) exists above one device.  Valid on plain
 * handles and on shard handles (ovqe_create_shard: the shard's rank bits enter every z parity).
 * R rotations exp(-i phi_r P_r) given in FORWARD order, masks on the handle's local bits (physical bit space), applied last to
 * first to the handle's state psi and to lam_dev (2^n_local complex amplitudes, same layout):
 *   w[r] = Im sum_i conj(lam_i) (P_r psi)_i  over this handle's amplitudes, on the states AFTER rotation r,
 *   then psi <- U_r^+ psi, lam <- U_r^+ lam.
 * Consecutive same-x runs whose x masks fit a tile are un-applied in ONE pass over both vectors (k_tile_adjoint: the psi and the
 * lambda tile in LDS; option "adjoint_tile_bits": -1 automatic, 11 / 12 the tile size, 0 one pass per run of at most 16 rotations);
 * ovqe_last_screen_support(which = 4 / 5) reports the passes and their bytes (64 per amplitude and pass).  The sums are reduced
 * in a fixed order.  Synchronises before it returns.
 * Refused under option "real_state" (OVQE_ERR_STATE) and when lam_dev is the state buffer. */
int ovqe_adjoint_rotations(ovqe_handle h, void *lam_dev, int64_t R, const uint64_t *x, const uint64_t *z,
                           const double *phi, double *w);

/* ---- lowest eigenpair of the stored Hamiltonian (Lanczos on the device, two-pass: tridiagonal matrix, then the Ritz
 * vector by the same recurrence; random start vector from `seed`, so every symmetry sector is reached — the global
 * minimum over the whole register, like column 0 of the reference's dense np.linalg.eigh,
 * ref:openvqe/adapt/fermionic_adapt_vqe.py:474 / qubit_adapt_vqe.py:424-426, which is O(8^n) and infeasible at the
 * H2O size).  Stops when the Lanczos residual estimate < tol * max(1, |lambda|) or after max_iter steps.  The
 * normalised eigenvector is left in the handle's state buffer (ovqe_get_state); *energy includes the constant,
 * *residual = |H y - lambda y| measured afterwards, *iterations = Lanczos steps taken. */
int ovqe_ground_state(ovqe_handle h, double tol, int max_iter, uint64_t seed, double *energy, double *residual,
                      int *iterations);
/* ... and of the Hamiltonian RESTRICTED TO THE SUPPORT of the stored program's states (sector tables, option "sector";
 * built by this call when they do not exist yet), inside the BLOCK OF THE REFERENCE DETERMINANT: the determinants that the
 * non-zero matrix elements connect to |hf> are found first and the Lanczos vectors live on them alone, so tables on a superset
 * of the symmetry sector (the one-angle-per-rotation probe of spin-adapted ansaetze lists several particle-number sectors)
 * give the same number as tables on the sector itself.  For a particle-number / spin conserving ansatz on a Hartree-Fock
 * determinant that is the full-CI energy of the determinant's symmetry sector — the `fci` argument the reference's
 * drivers take from PySCF (ref:openvqe/common_files/molecule_factory.py:120-125, `info["FCI"]`), here for active spaces the dense
 * routines cannot reach (N2/cc-pVDZ (10e,12o): 627 264 determinants, 538 M matrix elements).  Two-pass Lanczos on
 * vectors of |support| doubles, H v from the materialised matrix.  The normalised eigenvector is left in the handle's state
 * buffer (zeros outside the support: ovqe_get_state / ovqe_get_support).  OVQE_ERR_STATE when the program has no such tables
 * (not a real-amplitude program, support denser than 1/sector_sparsity, tables beyond sector_max_gb).
 * WITHOUT a stored program the sector is that of the state in the buffer: the closure of its support under the Hamiltonian's
 * x-groups — after ovqe_init_basis(hf) the (N_alpha, N_beta) sector of the reference determinant, with no UCCSD program to name it
 * (the tables are those of the ADAPT screens, option "screen_sector", and are kept for them). */
int ovqe_sector_ground_state(ovqe_handle h, double tol, int max_iter, uint64_t seed, double *energy, double *residual,
                             int *iterations);

/* ---- one- and two-particle reduced density matrices of the resident state psi (what a chemist takes from a converged wave function;
 * the reference takes a one-particle density from its PySCF run and diagonalises it to select active spaces by natural-orbital
 * occupations, ref:openvqe/common_files/molecule_factory_with_sparse.py:293-324).  CONVENTION: the register is read as n = n_qubits spin orbitals under the
 * JORDAN-WIGNER transform — the only encoding this call knows — with orbital p = reference qubit p = index bit n-1-p, and, for the
 * spin-resolved helpers of openvqe_amd/rdm.py, even orbitals alpha, odd orbitals beta (openvqe_amd/fermion.py spin_orbital_integrals).
 *   order 1: out = n*n complex (re,im), row-major  gamma[p][q] = <psi| a+_p a_q |psi>
 *   order 2: out = P*P complex, P = n(n-1)/2 pairs (p<q) in lexicographic order,
 *            D2[(p<q)][(r<s)] = <psi| a+_p a+_q a_s a_r |psi>,  so that  Gamma[p][q][r][s] = <a+_p a+_q a_r a_s> = -D2[(p,q)][(r,s)]
 * Both are Gram matrices (Hermitian — to the bit — and positive semidefinite) of rows v_K, one per register index K that lies one /
 * two annihilations below a non-zero amplitude:  v_K[a] = (-1)^{occ_K(t<a)} psi[K | bit(a)],  v_K[(a<b)] = (-1)^{occ_K(a<t<b)}
 * psi[K | bit(a) | bit(b)].  The rows are found from a bitmap of the support and materialised in chunks (option "rdm_workspace_mb");
 * a state without imaginary parts (every UCC / ADAPT / Lanczos state) runs in 8-byte arithmetic.  COST: the number of rows — for a
 * sparse state (a symmetry sector) a small multiple of its support, for a DENSE register 2^n rows of n or P entries each: the call
 * is meant for sparse states or small registers.  The state is only read; partial sums are reduced in a fixed order (bit-identical
 * results from call to call).  Synchronous.  Plain handles of any n >= 1; OVQE_ERR_INVALID for an order other than 1 or 2, order 2
 * with n < 2 and a NULL output; OVQE_ERR_STATE on a shard of a partitioned register and under option "real_state". */
int ovqe_rdm(ovqe_handle h, int order, double *out_re_im);
/* of the last ovqe_rdm call, up to `count` entries of: [0] non-zero amplitudes [1] rows [2] row chunks [3] 1 = real form [4] workspace bytes
 * [5] Gram launches [6] block pairs (64 x 64 outputs, upper triangle) [7] row slices per chunk  [8..11] HIP-event times in microseconds:
 * census + shadows + row list, rows kernels, Gram kernels, final reduction ([9..11] stay 0 beyond 64 chunks); zeros before the first call */
int ovqe_rdm_info(ovqe_handle h, int64_t *info, int count);

/* ---- Fubini-Study metric of the ansatz state (the real part of the quantum geometric tensor): with psi = U(theta)|hf> of the stored
 * program and the tangent vectors T_k = d psi / d theta_k,
 *   metric[K*K], row-major:  g_ij = Re( <T_i|T_j> - <T_i|psi><psi|T_j> )      K x K, real, symmetric, positive semidefinite
 * — the ingredient of natural-gradient descent / imaginary-time evolution (the gradient-descent optimiser with natural_gradient=True
 * of the qat-variational package the reference's requirements pin; openvqe_amd/common_files/natural_gradient.py is its counterpart here).
 * CONTRACT.  The angle of rotation r is coeff_r theta[pidx_r] + phi0_r (of a gate: ascale theta[pidx] + aconst), so
 *   T_k = sum_{r: pidx_r = k} coeff_r U_{>r} (-i P_r) U_{<=r} |hf>      (RX / RY / RZ: the factor -i/2 with the gate's axis, and ascale);
 * a parameter shared by several rotations sums their contributions; a parameter no rotation uses, or a rotation with pidx < 0, gives a
 * zero row and column.  Gate programs in Clifford-frame form are evaluated on the frame state: the net Clifford operator is a fixed
 * unitary and drops out of g.  The result is symmetric to the bit and bit-identical from call to call (fixed-order reductions, no
 * atomics).  The state buffer is unspecified after the call (as after ovqe_energy); cached tables of the handle stay valid: an
 * ovqe_energy before the call and one after it return the same bits.  No Hamiltonian is needed.
 * TWO PATHS (ovqe_metric_info [0]).  1, compact support: a real-amplitude program (every string an odd number of Y, no literal gate left)
 * whose reachable support holds at most 4096 basis states (the H2O / LiH class) — one workgroup per parameter carries psi and its tangent
 * through the program's pair lists in LDS, one launch for all K tangents, then the Gram matrix of the tangents (<psi|T_k> = 0 on a
 * real state).  2, streaming (any other program, option "force_path" = 2): psi and the K tangents as columns of a store of 2^n rows behind
 * option "metric_workspace_mb"; the op list is walked once, every op applied to psi and all live tangents in one launch, behind each
 * parameterised rotation its tangent takes coeff (-i P) psi; then the Gram matrix and the <T_i|psi> correction.  COST of path 2:
 * O(K R) sweeps of the register for R rotations — meant for small registers and short programs.  Out of scope: tangents on the sector
 * tables and the partitioned register (24-qubit N2 with 1715 parameters is answered OVQE_ERR_ALLOC).
 * OVQE_ERR_STATE with no program set, on a shard of a partitioned register and under option "real_state"; OVQE_ERR_INVALID for a K other
 * than the program's, a NULL theta or metric (K = 0: only metric is checked); OVQE_ERR_ALLOC, with the bytes needed in the text, when
 * the tangent store does not fit its cap. */
int ovqe_metric_tensor(ovqe_handle h, const double *theta, int32_t K, double *metric);
/* of the last ovqe_metric_tensor call, up to `count` entries of: [0] path (1 compact support, 2 streaming) [1] K [2] amplitudes per tangent
 * [3] bytes of the tangent store [4] launches of the tangent stage [5] Gram launches [6..8] HIP-event times in microseconds: tangents,
 * Gram, finish [9] form of the tangent kernel: 0 streaming, 1 compact with ops and pair words staged in LDS, 2 compact with both read
 * from global memory [10] dynamic LDS bytes of the tangent launch (0 on the streaming path); zeros before the first call */
int ovqe_metric_info(ovqe_handle h, int64_t *info, int count);

/* ---- exact energy Hessian of the stored program: with E(theta) = <psi(theta)|H|psi(theta)> of the stored Hamiltonian,
 *   hess[K*K], row-major:  d2E / dtheta_i dtheta_j      K x K, real, symmetric to the bit
 * together with E (energy, may be NULL) and the gradient (grad[K], may be NULL) of the same point — what decides whether a converged point
 * is a minimum (lowest eigenvalue) and what Newton / trust-region optimisers step with (openvqe_amd/common_files/newton.py).  Forward
 * over reverse: the adjoint pass of ovqe_energy_gradient differentiated in every direction b, with the tangents of ovqe_metric_tensor
 * (the derivation: openvqe_amd/csrc/sv_hessian_host.hpp).  Row b of the raw matrix M comes from direction b and M is symmetric to
 * rounding only: the call returns (M + M^T) / 2 and reports max |M - M^T| in *asymmetry (may be NULL) as a built-in self-check.
 * CONTRACT (ovqe_metric_tensor's).  The angle of rotation r is coeff_r theta[pidx_r] + phi0_r; a parameter shared by several rotations
 * sums their contributions; a parameter no rotation uses, or a rotation with pidx < 0, gives a zero row and column.  A Hamiltonian must be
 * set.  Gate programs whose Clifford frame is open are evaluated with the conjugated Hamiltonian, as by ovqe_energy.  The state buffer is
 * unspecified after the call; cached tables of the handle stay valid: an ovqe_energy before the call and one after it return the same bits.
 * TWO PATHS (ovqe_hessian_info [0]).  1, compact support: a real-amplitude program whose reachable support holds at most 4096 basis states
 * and whose four LDS vectors (psi, tangent, lambda = H psi, mu = H tangent) and tables fit one workgroup: ONE launch, one 64-lane workgroup
 * per direction, the real part of the Hamiltonian restricted to the support.  LDS atomics add lambda, mu and the weights as in the compact
 * gradient kernel: the result reproduces to rounding, not to the bit.  2, streaming (any other program, option "force_path" = 2, or a
 * compact program too large for LDS): psi and the K tangents as columns of a store of 2^n rows and a second store of their images
 * under H, both behind option "metric_workspace_mb"; the op list is walked backwards on both, fixed-order sums, bit-identical from call
 * to call.  COST of path 2: O(K R) sweeps of the register for R rotations — meant for small registers and short programs.  Out of scope:
 * the sector tables and the partitioned register.
 * OVQE_ERR_STATE with no program or no Hamiltonian set, on a shard of a partitioned register and under option "real_state";
 * OVQE_ERR_INVALID for a K other than the program's, a NULL theta or hess (K = 0: only hess is checked; the energy alone is answered);
 * OVQE_ERR_ALLOC, with the bytes needed in the text, when the workspace does not fit the cap of option "metric_workspace_mb". */
int ovqe_energy_hessian(ovqe_handle h, const double *theta, int32_t K, double *energy, double *grad, double *hess, double *asymmetry);
/* of the last ovqe_energy_hessian call, up to `count` entries of: [0] path (1 compact support, 2 streaming) [1] K [2] amplitudes per vector
 * [3] workspace bytes (path 1: the rows, gradient and energy and the restricted Hamiltonian; path 2: both stores, the slab sums and the
 * weight records) [4] launches [5] entries of the restricted Hamiltonian (path 1) [6..8] HIP-event times in microseconds: path 1 the
 * copy of theta to the device together with the one launch, the copy back, 0 (no third phase); path 2 tangents and H images, the
 * backward walk, the copy back [9] kernel form: 0 streaming, 1 compact with
 * ops and pair words staged in LDS, 2 compact with both read from global memory [10] dynamic LDS bytes of the launch (0 on the streaming
 * path); zeros before the first call */
int ovqe_hessian_info(ovqe_handle h, int64_t *info, int count);

/* ---- exact gradients of a BATCH of parameter vectors: row b of theta[B x K] (row-major) gives energies[b] and grads[b*K .. b*K + K), what
 * ovqe_energy_gradient(h, theta + b*K, K, ...) answers on the same handle — what a multi-start optimisation asks for in every iteration
 * (openvqe_amd/common_files/multistart.py).  ROWS.  The single call's conventions: a parameter shared by several rotations sums their
 * contributions, a parameter no rotation uses gives exact zeros, a gate program whose Clifford frame is open is evaluated with the
 * conjugated Hamiltonian.  Rows do not influence each other.  REFUSALS.  Whatever ovqe_energy_gradient refuses (no program, no
 * Hamiltonian: OVQE_ERR_STATE; K other than the program's, a shard handle: OVQE_ERR_INVALID; ...) is refused with the same code;
 * B < 0 and a NULL theta / energies / grads with B K > 0 (energies: B > 0) give OVQE_ERR_INVALID; B = 0 returns OVQE_OK and touches
 * nothing.  BOUNDS.  B K doubles of theta are read; B doubles of energies and B K of grads are written.  AFTER THE CALL the state
 * buffer is unspecified, as after ovqe_energy; cached tables stay valid: ovqe_energy and ovqe_energy_batch before and after return the
 * same bits.  Synchronises before it returns.
 * TWO PATHS (ovqe_gradient_batch_info [0]).  1, compact support: the program whose single gradient runs in a one-wave form on the compact
 * support — a compact program exists, at most 16 qubits, option "force_path" 0 or 3, option "sparse_grad" on, and psi, lambda, the
 * cos/sin table and the weights of one wave within 150 KiB of LDS.  Nothing is planned or built: the tables are the single call's.  The
 * whole batch runs in ONE launch of k_sparse_grad_batch: workgroups of 1, 2, 4 or 8 waves, a wave per row at a time, one copy of the op
 * records and pair words per workgroup (staged in LDS, or read from global memory where they do not fit); geometry by
 * openvqe_amd/csrc/sv_gradbatch_host.hpp, options "grad_batch_waves" and "grad_batch_workgroups".  The energy of a row is summed in a fixed
 * order: equal rows give bit-identical energies wherever they sit in the batch.  LDS atomics add lambda and the weights as in the
 * single kernel: gradients reproduce to rounding.  2, every other program (sector tables, streaming, literal gate lists): the rows one
 * by one through the body of ovqe_energy_gradient.  Out of scope: batched forms of the sector and the streaming paths.
 * Everything the call allocates is its own: the buffers of the energy paths are not touched. */
int ovqe_energy_gradient_batch(ovqe_handle h, int64_t B, const double *theta, int32_t K, double *energies, double *grads);
/* of the last ovqe_energy_gradient_batch call with B > 0, up to `count` entries of: [0] path (1 compact support, 2 row by row) [1] B [2] K
 * [3] launches (path 1: 1; path 2: 0 — the single call's launches are not counted) [4] kernel form: 1 ops and pair words staged in LDS, 2
 * read from global memory, 0 on path 2 [5] waves per workgroup [6] workgroups [7] dynamic LDS bytes of the launch [8] support size m
 * [9] [10] HIP-event times in microseconds: the copy of theta to the device with the launch, the copy back ([4..10] are 0 on path 2);
 * zeros before the first call */
int ovqe_gradient_batch_info(ovqe_handle h, int64_t *info, int count);

/* ---- variational quantum deflation (VQD): excited states as minima of C(theta) = <psi(theta)|H|psi(theta)> + sum_j beta_j |<phi_j|psi(theta)>|^2
 * with the states phi_j found so far (openvqe_amd/excited.py: vqd).  The penalty is the rank-J operator sum_j beta_j |phi_j><phi_j| beside
 * H: the adjoint gradient is the pass of ovqe_energy_gradient with lambda = H psi + sum_j beta_j phi_j <phi_j|psi>.
 *
 * ovqe_deflation_push: a copy of the 2^n complex amplitudes in the state buffer becomes vector J of the handle, J the number held so
 * far, with weight beta — whatever the buffer holds: the result of ovqe_prepare_state, a Lanczos eigenvector, a Ritz state, what
 * ovqe_set_state wrote.  The vector is taken as it is, not normalised.  The state buffer is only read: the same bits afterwards.  The
 * vectors belong to the REGISTER, not to a program: they survive ovqe_set_program, ovqe_set_gate_program and ovqe_set_hamiltonian.  At
 * most 32 are held, each 16 * 2^n bytes of device memory owned by the handle (freed by ovqe_deflation_truncate and ovqe_destroy).
 * OVQE_ERR_INVALID for a beta that is not finite or negative and for a 33rd vector; OVQE_ERR_STATE on a shard of a partitioned
 * register and under option "real_state"; OVQE_ERR_ALLOC, with the bytes needed in the text, when the vector is more than 60 % of the
 * free device memory.  Synchronises before it returns. */
int ovqe_deflation_push(ovqe_handle h, double beta);
/* keeps the first `count` vectors and frees the others; 0 clears the set.  OVQE_ERR_INVALID for a count outside 0 .. the number held. */
int ovqe_deflation_truncate(ovqe_handle h, int32_t count);
/* *count = the number of vectors held */
int ovqe_deflation_count(ovqe_handle h, int32_t *count);
/* DEFLATED energies and gradients of a batch: for row b of theta[B x K] (row-major), with psi = psi(theta_b) of the stored program and
 * the J vectors held,
 *     o_bj = <phi_j|psi>,   energies[b] = <psi|H|psi> + constant,   costs[b] = energies[b] + sum_j beta_j |o_bj|^2,
 *     grads[b*K .. b*K + K) = dC/dtheta,   overlaps_re_im = the B x J complex o_bj, row-major, (re, im) pairs.
 * energies and overlaps_re_im may be NULL.  With no vector held the call is valid: costs equal energies to the bit, overlaps_re_im is
 * not touched.  ROWS.  The conventions of ovqe_energy_gradient_batch: a shared parameter sums its rotations' contributions, an unused
 * one gives exact zeros, rows do not influence each other.  REFUSALS.  Those of ovqe_energy_gradient_batch with its codes and texts,
 * `costs` in the place of its `energies`: no program, no Hamiltonian: OVQE_ERR_STATE; K other than the program's, a shard handle, B < 0,
 * a NULL theta / costs / grads with B K > 0 (costs: B > 0): OVQE_ERR_INVALID; B = 0 returns OVQE_OK and touches nothing.  Further:
 * OVQE_ERR_STATE under option "real_state", and for a gate program whose Clifford frame is OPEN — the vectors live in the caller's
 * frame, the state such a program evaluates does not; option "clifford_frame" = 0 runs such a list literally.  BOUNDS.  B K doubles of
 * theta are read; B doubles of costs (and of energies), B K of grads and 2 B J of overlaps_re_im are written.  AFTER THE CALL the state
 * buffer is unspecified; cached tables stay valid: ovqe_energy, ovqe_energy_batch and ovqe_energy_gradient before and after return what
 * they returned.  Synchronises before it returns.
 * TWO PATHS (ovqe_deflation_info [0]).  1, compact support: exactly the programs ovqe_energy_gradient_batch runs on its path 1, planned by
 * the same rule under the same options ("grad_batch_waves", "grad_batch_workgroups"), the whole batch in ONE launch of
 * k_sparse_vqd_batch: the row body of k_sparse_grad_batch with one phase between lambda = H psi and the backward walk.  The vectors
 * enter as REAL rows over the slots of the compact state, read from global memory (no LDS beyond that kernel's): Re phi_j restricted to
 * the support, and Im phi_j as a second row with the same weight when it is non-zero anywhere on the support; psi is zero off the
 * support, so the restriction is exact.  The rows are gathered by k_deflate_gather and cached on the handle until the compact program
 * is rebuilt or the set of vectors changes.  Cost, energy and overlaps of a row are summed in fixed orders: equal rows give
 * bit-identical costs, energies and overlaps wherever they sit in the batch; LDS atomics add lambda and the weights as in the single
 * kernel: gradients reproduce to rounding.  2, streaming — every other program, those that otherwise run on the sector tables
 * included, and literal gate lists: row by row psi = U(theta)|hf> on the streaming kernels, lambda = H psi, the overlaps four vectors per
 * pass over psi (k_deflate_dots: per-workgroup partials summed in a fixed order, bit-identical from call to call), lambda += sum_j
 * beta_j o_j phi_j four vectors per pass (k_deflate_axpy), then the backward walk of ovqe_energy_gradient.  COST of path 2 beyond the
 * single gradient: J extra reads of 16 * 2^n bytes for the overlaps and J more for lambda, per row.  Out of scope: deflation on the
 * sector tables and on the partitioned register, open Clifford frames, a deflated Hessian or metric. */
int ovqe_deflated_gradient_batch(ovqe_handle h, int64_t B, const double *theta, int32_t K, double *costs, double *grads, double *energies,
                                 double *overlaps_re_im);
/* of the last ovqe_deflated_gradient_batch call with B > 0, up to `count` entries of: [0] path (1 compact support, 2 streaming) [1] B [2] K
 * [3] J, the vectors held [4] real rows of path 1 (J + the vectors with an imaginary part on the support; 0 on path 2) [5] launches
 * (path 1: 1; path 2: the k_deflate_dots, k_reduce and k_deflate_axpy launches of all rows — those of the single gradient are not
 * counted) [6] kernel form: 1 ops and pair words staged in LDS, 2 read from global memory, 0 on path 2 [7] waves per workgroup
 * [8] workgroups [9] dynamic LDS bytes of the launch [10] support size m [11] gather launches of this call (0: the cached rows served)
 * [12] [13] HIP-event times in microseconds: the copy of theta to the device with the launch, the copy back ([6..13] are 0 on path 2);
 * zeros before the first call; a refused call leaves no figures */
int ovqe_deflation_info(ovqe_handle h, int64_t *info, int count);

/* ---- energy spread: how good a state is, and the folded-spectrum cost.  For psi = psi(theta_b) and a reference energy omega_b,
 *     S_b = ||(H - omega_b) psi||^2 = <psi|(H - omega_b)^2|psi>        (H with its constant)
 * With omega_b = E_b = <psi|H|psi> it is the energy VARIANCE <H^2> - <H>^2: zero exactly on eigenstates, and an eigenvalue of H lies
 * within sqrt(S_b) of E_b (Weinstein).  With a chosen omega it is the folded-spectrum cost: its minimum over theta is the ansatz state
 * nearest the energy omega — excited states without stored deflation vectors (openvqe_amd/excited.py: folded_spectrum).
 *
 * ovqe_spread_gradient_batch: for row b of theta[B x K] (row-major),
 *     energies[b] = E_b,   spreads[b] = S_b,   costs[b] = w_energy E_b + w_spread S_b,
 *     grads[b*K .. b*K + K) = d costs[b] / dtheta at FIXED omega_b.
 * omega: B values, or NULL for omega_b = E_b — then the gradient is the exact gradient of w_energy E + w_spread Var, because
 * d(<H^2> - E^2) = d<H^2> - 2 E dE is what fixing omega at E gives.  The adjoint pass is ovqe_energy_gradient's with
 * lambda = w_energy H psi + w_spread (H - omega)^2 psi (components of lambda along psi contribute nothing).  energies and spreads may
 * be NULL.  ROWS.  The conventions of ovqe_energy_gradient_batch: a shared parameter sums its rotations' contributions, an unused one
 * gives exact zeros, rows do not influence each other.  REFUSALS.  Those of ovqe_deflated_gradient_batch with its codes, without the
 * one for open Clifford frames — the conjugated Hamiltonian squares like any other: no program, no Hamiltonian, option "real_state":
 * OVQE_ERR_STATE; K other than the program's, a shard handle, B < 0, a NULL theta / costs / grads with B K > 0 (costs: B > 0), a
 * weight or an omega_b that is not finite: OVQE_ERR_INVALID; B = 0 returns OVQE_OK and touches nothing.  BOUNDS.  B K doubles of theta
 * and B of omega are read; B doubles of costs (and of energies, of spreads) and B K of grads are written.  AFTER THE CALL the state
 * buffer is unspecified; cached tables stay valid: ovqe_energy, ovqe_energy_batch and ovqe_energy_gradient before and after return what
 * they returned.  Synchronises before it returns.
 * TWO PATHS (ovqe_spread_info [0]).  1, compact support: the whole batch in ONE launch of k_sparse_spread_batch — the row body of
 * k_sparse_grad_batch with a third per-wave LDS array and one phase between lambda = H psi and the backward walk: sigma = (H - omega) psi
 * in place, S = sum sigma_i^2, mu = (H - omega) sigma by a second pass over the restricted Hamiltonian's entries, lambda from both.
 * Taken when ovqe_energy_gradient_batch would take its path 1, AND the three-array region of one wave fits 150 KiB, AND the restricted
 * entries are H on the support: the compact program drops what leaves the support and every term with an odd number of Y — exact for
 * <H> on a real state, wrong for <H^2> — so path 1 requires that no term with a non-zero coefficient has an odd number of Y, and that
 * for every x-group and every support state whose partner lies outside the support the group's signed coefficient sum is at most
 * 64 eps sum_t |c_t| in magnitude (the residue a number-conserving Hamiltonian leaves there: 1e-17 .. 3e-16, not 0).  Both are decided
 * once, when the compact program is built.  Planned by ovqe_energy_gradient_batch's rule on the larger layout under the same options
 * ("grad_batch_waves", "grad_batch_workgroups").  With w_energy = 1, w_spread = 0 costs and energies equal ovqe_energy_gradient_batch's
 * to the bit.  E and S of a row are summed in fixed orders: equal rows give bit-identical energies and spreads wherever they sit in the
 * batch; LDS atomics add lambda, mu and the weights: gradients reproduce to rounding.  2, streaming — every other program: sector-table
 * and dense programs, literal gate lists, Hamiltonians that leak from the support or hold odd-Y terms, "force_path" 2: row by row
 * psi = U(theta)|hf> on the streaming kernels, sigma and tau = (H - omega) sigma by the Pauli-sum application on the full complex
 * register in two register-sized work vectors the call allocates and frees (OVQE_ERR_ALLOC when it cannot), the dot products by the
 * fixed-order reductions, then the backward walk of ovqe_energy_gradient.  COST of path 2 beyond the single gradient: one more
 * Pauli-sum application and six vector passes per row.  Out of scope: batched forms on the sector tables and on the partitioned
 * register, a spread Hessian. */
int ovqe_spread_gradient_batch(ovqe_handle h, int64_t B, const double *theta, int32_t K, const double *omega, double w_energy, double w_spread,
                               double *costs, double *grads, double *energies, double *spreads);
/* of the last ovqe_spread_gradient_batch call with B > 0, up to `count` entries of: [0] path (1 compact support, 2 streaming) [1] B [2] K
 * [3] mode (0: omega given, 1: variance) [4] launches (path 1: 1; path 2: the vector operations of all rows beyond the single gradient's
 * — the Pauli-sum applications are not counted) [5] kernel form: 1 ops and pair words staged in LDS, 2 read from global memory, 0 on
 * path 2 [6] waves per workgroup [7] workgroups [8] dynamic LDS bytes of the launch [9] support size m [10] why path 2 served the call:
 * 0 it did not, 1 no compact program or the options rule it out, 2 the three-array region exceeds the LDS budget, 3 the Hamiltonian
 * leaks from the support, 4 it holds a term with an odd number of Y [11] [12] HIP-event times in microseconds: the copy of theta to the
 * device with the launch, the copy back ([5..9], [11], [12] are 0 on path 2); zeros before the first call; a refused call leaves no
 * figures */
int ovqe_spread_info(ovqe_handle h, int64_t *info, int count);

/* ---- observables beside the Hamiltonian: expectation values of a batch, penalty terms, constrained costs.  A handle holds up to 8
 * further Hermitian Pauli sums O_m.  For psi = psi(theta_b), o_bm = <psi|O_m|psi> + constant_m, and the cost of a row is
 *     costs[b] = E_b + sum_m [ linear_m o_bm + quad_m (o_bm - target_m)^2 ] + sum_j beta_j |<phi_j|psi>|^2
 * with the deflation vectors phi_j the handle holds (ovqe_deflation_push).  For any cost f(E, o_1 .. o_M) the adjoint vector is
 * lambda = H psi + sum_m (df/do_m) O_m psi: one pass of ovqe_energy_gradient gives cost, exact gradient, E and every o_bm.  Uses: a
 * spin penalty quad (<S^2> - s(s+1))^2 that makes VQD return states of one spin (openvqe_amd/excited.py: vqd(constraints=...),
 * spin_constraint), a particle-number penalty for ansaetze that do not conserve N, properties of a batch of states without a table
 * rebuild per observable.
 *
 * ovqe_observable_push: arguments as ovqe_set_hamiltonian, coefficients real; the sum becomes observable M of the handle, M the number
 * held so far.  The observables belong to the REGISTER, as the deflation vectors do: they survive ovqe_set_program,
 * ovqe_set_gate_program and ovqe_set_hamiltonian.  OVQE_ERR_INVALID for a ninth observable, a mask beyond the register, a coefficient
 * or constant that is not finite; OVQE_ERR_STATE on a shard of a partitioned register and under option "real_state".  Synchronises. */
int ovqe_observable_push(ovqe_handle h, int64_t T, const uint64_t *x, const uint64_t *z, const double *coeff, double constant);
/* keeps the first `count` observables and frees the others; 0 clears the set.  OVQE_ERR_INVALID for a count outside 0 .. the number held. */
int ovqe_observable_truncate(ovqe_handle h, int32_t count);
/* *count = the number of observables held */
int ovqe_observable_count(ovqe_handle h, int32_t *count);
/* CONSTRAINED costs and gradients of a batch: for row b of theta[B x K] (row-major), with the M observables and the J vectors held,
 *     energies[b] = E_b,   values[b*M + m] = o_bm,   costs[b] as above,   grads[b*K .. b*K + K) = d costs[b] / dtheta,
 *     overlaps_re_im = the B x J complex <phi_j|psi>, row-major, (re, im) pairs.
 * M must equal the number of observables held.  linear, quad, target: M doubles each; a NULL linear or quad means zeros, a NULL target
 * zeros; with both weights NULL the call returns the expectation values of a batch (costs = the deflated cost).  energies, values
 * and overlaps_re_im may be NULL.  With no observable and no vector held costs equal energies to the bit.  ROWS.  The conventions of
 * ovqe_energy_gradient_batch.  REFUSALS.  Those of ovqe_deflated_gradient_batch with its codes — no program, no Hamiltonian, option
 * "real_state", an OPEN Clifford frame (the observables and vectors live in the caller's frame, the state of an open-frame program does
 * not): OVQE_ERR_STATE; K other than the program's, a shard handle, B < 0, a NULL theta / costs / grads with B K > 0 (costs: B > 0):
 * OVQE_ERR_INVALID — and: M other than the number held, a weight or target that is not finite: OVQE_ERR_INVALID.  B = 0 returns
 * OVQE_OK and touches nothing.  BOUNDS.  B K doubles of theta and M of each of linear, quad, target are read; B doubles of costs (and
 * of energies), B K of grads, B M of values and 2 B J of overlaps_re_im are written.  AFTER THE CALL the state buffer is unspecified;
 * cached tables stay valid: ovqe_energy, ovqe_energy_gradient, ovqe_energy_gradient_batch, ovqe_deflated_gradient_batch and
 * ovqe_spread_gradient_batch before and after return what they returned.  Synchronises before it returns.
 * TWO PATHS (ovqe_constraint_info [0]).  1, compact support: taken exactly when ovqe_deflated_gradient_batch takes its path 1, planned by
 * the same rule under the same options, the whole batch in ONE launch of k_sparse_constrained_batch: k_sparse_vqd_batch's row body with
 * one more phase behind the deflation phase.  Every O_m enters RESTRICTED to the support, by the rule that restricts H
 * (sv_constrain_host.hpp): entries whose partner leaves the support and terms with an odd number of Y are dropped.  That is exact for
 * o_bm and its gradient — the ket side of the backward walk never leaves the support, and an odd-Y term has no expectation value on a
 * real state and adds only an imaginary vector to lambda — so, unlike ovqe_spread_gradient_batch, there is no exactness gate.  The
 * entries of all observables are one array in global memory (no LDS beyond the batched gradient's), built lazily and cached on the
 * handle until the compact program is rebuilt or the set of observables changes.  Per observable one pass over its entries sums o_bm;
 * where g = linear_m + 2 quad_m (o_bm - target_m) is not zero a second pass adds g O_m psi to lambda.  Cost, energy, values and
 * overlaps of a row are summed in fixed orders: equal rows give bit-identical costs, energies, values and overlaps wherever they sit
 * in the batch; gradients reproduce to rounding.  2, streaming — every other program and "force_path" 2: ovqe_deflated_gradient_batch's
 * row with, per observable, work = O_m psi by the Pauli-sum application in ONE register-sized work vector the call allocates and frees
 * (OVQE_ERR_ALLOC when it cannot), o_bm by the fixed-order dot product, lambda += g work, then the backward walk.  COST of path 2 beyond
 * the deflated row: M Pauli-sum applications and up to 2 M vector passes.  Out of scope: constraints on the sector tables and on the
 * partitioned register, open Clifford frames, a constrained Hessian or metric, per-row weights. */
int ovqe_constrained_gradient_batch(ovqe_handle h, int64_t B, const double *theta, int32_t K, int32_t M, const double *linear, const double *quad,
                                    const double *target, double *costs, double *grads, double *energies, double *values,
                                    double *overlaps_re_im);
/* of the last ovqe_constrained_gradient_batch call with B > 0, up to `count` entries of: [0] path (1 compact support, 2 streaming) [1] B
 * [2] K [3] M [4] J, the vectors held [5] real deflation rows of path 1 [6] launches (path 1: 1; path 2: the deflation launches and the
 * observables' k_dot, k_reduce and axpy launches of all rows — Pauli-sum applications and the single gradient's are not counted)
 * [7] kernel form: 1 ops and pair words staged in LDS, 2 read from global memory, 0 on path 2 [8] waves per workgroup [9] workgroups
 * [10] dynamic LDS bytes of the launch [11] support size m [12] entries of all restricted observables [13] observables restricted by
 * this call (0: the cached entries served) [14] [15] HIP-event times in microseconds: the copy of theta to the device with the launch,
 * the copy back ([7..15] are 0 on path 2); zeros before the first call; a refused call leaves no figures */
int ovqe_constraint_info(ovqe_handle h, int64_t *info, int count);

/* ---- finite-shot measurement: outcomes drawn from the state in the buffer, and energies with shot noise (what a submission with
 * nbshots > 0 asks of a QPU: openvqe_amd/qat_compat.py; every call site of the reference submits nbshots = 0, the exact paths above).
 * Plain handles of any size; OVQE_ERR_STATE on a shard of a partitioned register and under option "real_state".  The state buffer is
 * only read: psi is the same to the bit afterwards.
 *
 * UNIFORMS.  With mix64 the hash of ovqe_randomize (openvqe_amd/synth.py restates both on the host, bit for bit):
 *     key = mix64(seed ^ mix64(stream)),    u(s) = (mix64(key ^ mix64(s)) >> 11) * 2^-53  in [0, 1),    s the ABSOLUTE shot number.
 * Shots [0, S) drawn in one call or in pieces (first_shot) are the same bits; (seed, stream) pairs give independent sequences.
 *
 * OUTCOME OF A SHOT.  p_i = |a_i|^2, W = sum_i p_i (the state need not be normalised; W = 0 or not finite: OVQE_ERR_STATE), C_i the
 * inclusive prefix sum of p in index order: the outcome is the smallest i with C_i > u W.  The device sums C in a fixed blocked order,
 * so the same call returns the same bits every time and C agrees with the exact prefix sums to (2^n - 1) 2^-53 W; an index with
 * p_i = 0 is never returned (zero entries are marked in the prefix array and stepped over, also for u close to 1 on a state whose tail
 * is zero).  Outcome bit (n-1-q) is qubit q's result, bit 1 <-> eigenvalue -1.
 *
 * BASIS.  xbasis / ybasis: disjoint masks of index bits inside the register (else OVQE_ERR_INVALID), measured in X / in Y; the other
 * bits in Z.  Outcomes are drawn from |phi|^2, phi = B psi, B the tensor product of H on the x bits and H S^+ on the y bits:
 * (|0> + i|1>)/sqrt 2 measured in Y gives bit 0.  phi lives in scratch: 8 * 2^n bytes for the prefix array, 16 * 2^n more once a
 * rotated bit lies above the 2^11-amplitude tile of the basis-change kernel; allocated at first use and kept on the handle,
 * OVQE_ERR_ALLOC with the byte count in the text when that would take more than 60 % of the free device memory.
 *
 * indices[k] receives the outcome of shot first_shot + k, k < n_shots (0 <= n_shots <= 2^31). */
int ovqe_sample(ovqe_handle h, int64_t n_shots, uint64_t seed, uint64_t stream, uint64_t first_shot, uint64_t *indices);
/* the same shots in the given basis, scored on T diagonal terms: with b_s the outcome of shot s,
 *     term_sums[t] = sum_s (-1)^popcount(b_s & mask[t])   (integers, exact),
 *     value_sums   = { sum_s v_s, sum_s v_s^2 },   v_s = sum_t coeff[t] (-1)^popcount(b_s & mask[t]),
 * both sums in a fixed order (integer atomics, a fixed tree over the waves): bit-identical from call to call.  For a Pauli string
 * (x, z) that the basis diagonalises, mask = x | z; whether a term is diagonal in the basis is the caller's business.  indices may
 * be NULL (the outcomes are then not stored); T = 0 with no basis change is ovqe_sample. */
int ovqe_measure_paulis(ovqe_handle h, uint64_t xbasis, uint64_t ybasis, int64_t n_shots, uint64_t seed, uint64_t stream,
                        uint64_t first_shot, int64_t T, const uint64_t *mask, const double *coeff, int64_t *term_sums,
                        double *value_sums, uint64_t *indices);
/* the measurement plan of the stored Hamiltonian (OVQE_ERR_STATE without one), built once per Hamiltonian and kept on the handle.
 * A term acts on bit b with X if x & ~z, Y if x & z, Z if z & ~x.  Identity terms go to the constant and get group -1.  The others
 * are taken by |coeff| descending, ties by stored position; each goes into the FIRST group whose basis agrees with the term on every
 * bit where both act (qubit-wise commutation), and joining extends that group's basis; groups are numbered in creation order.
 * *n_groups receives the number of groups G; group_of_term takes up to `capacity` of the T entries, xbasis / ybasis up to `capacity`
 * of the G (G <= T; the arrays may be NULL when capacity is 0). */
int ovqe_measure_groups(ovqe_handle h, int64_t capacity, int32_t *group_of_term, uint64_t *xbasis, uint64_t *ybasis,
                        int64_t *n_groups);
/* <H> of the stored program at theta from n_shots shots PER GROUP of that plan.  Leaves U(theta)|hf> in the state buffer exactly as
 * ovqe_prepare_state does, then measures group g with stream = g, shots 0 .. n_shots - 1:
 *     energy = constant + sum_g mean_g,    std_error = sqrt(sum_g s_g^2 / n_shots),
 * mean_g and s_g^2 the mean and the unbiased sample variance of v over the shots of group g (a variance that rounding leaves below
 * zero counts as zero; equal values over a power-of-two number of shots give exactly zero).  n_shots < 2: OVQE_ERR_INVALID; no
 * Hamiltonian or no program: OVQE_ERR_STATE.  One wait for the whole call. */
int ovqe_energy_sampled(ovqe_handle h, const double *theta, int32_t K, int64_t n_shots, uint64_t seed, double *energy,
                        double *std_error);
/* of the last measuring call, up to `count` entries of: [0] groups measured (1 for ovqe_sample / ovqe_measure_paulis) [1] shots per
 * group [2] scratch bytes held [3] kernel launches [4..6] HIP-event times in microseconds summed over the groups: basis change,
 * scan, draw + score [7] terms scored [8] streaming passes for rotated bits above the tile; zeros before the first call */
int ovqe_measure_info(ovqe_handle h, int64_t *info, int count);

/* ---- excited states by subspace expansion (quantum subspace expansion; with an excitation pool the qEOM family): around the resident
 * state psi, with m = n_ops expansion operators O_j given as Pauli sums in the CSR form of ovqe_pool_gradients (operator k = terms
 * [offsets[k], offsets[k+1]), complex coefficients, strings as in ovqe_apply_pauli_sum: x & z = Y with its i^ny phase, x = z = 0 the
 * identity; an operator without terms is allowed and gives a zero row and column),
 *   phi_j = O_j psi,    s_out[i*m + j] = <phi_i|phi_j>,    h_out[i*m + j] = <phi_i|H|phi_j>        m x m complex (re,im), row-major
 * with H the stored Hamiltonian INCLUDING its constant (constant * S_ij), as ovqe_ground_state reports energies.  The generalised
 * eigenproblem H y = E S y is the caller's (openvqe_amd/excited.py); the reference's only excited-state code is a weighted
 * subspace-search demo on an Ising chain (ref:openvqe/common_files/get_energy_WSSVQE.py) and has no call site for this.
 * s_out is Hermitian to the bit with a real diagonal (upper triangle mirrored).  h_out holds all m^2 entries of Phi^H (H Phi) AS
 * COMPUTED — Hermitian up to rounding, the caller symmetrises.  h_out may be NULL: only S is formed, the sigma stage and its half of
 * the store are skipped and no Hamiltonian is needed.
 * STAGES (ovqe_subspace_info).  Rows R = { i : psi[i ^ x] != 0 for some distinct x mask of the pool }, a superset of every supp(phi_j),
 * from the bitmap of psi's support; the expansion vectors into an index-major store of |R| rows (16-byte amplitudes; columns [0, m) phi_j,
 * padded to mb = m rounded up to 64, then columns [mb, mb + m) sigma_j); sigma_j = H phi_j ON R — per row the coefficient of every
 * x-group of H once, applied to the m contiguous columns of the partner row; a partner outside R holds exact zeros and rows outside R
 * are never needed, since H_ij only sums over rows where phi_i is non-zero; then 64 x 64 Gram blocks of (Phi, Phi) and (Phi, Sigma) —
 * never (Sigma, Sigma).  When R is the whole register the row lookup is skipped (dense form).
 * COST.  The store is |R| * wpad * 16 bytes, wpad = 2 mb (mb when h_out is NULL), behind option "subspace_workspace_mb"; sigma costs
 * (matrix elements of H inside R) x m complex FMAs; the Gram stage |R| * 3/2 mb^2.
 * psi is only read: the state buffer holds the same bits afterwards.  Cached tables of the handle stay valid: an ovqe_energy before
 * the call and one after it return the same bits.  All reductions run in a fixed order without atomics: two calls return identical
 * bits.  Synchronous.  OVQE_ERR_STATE: h_out given but no Hamiltonian set, a shard of a partitioned register, option "real_state";
 * OVQE_ERR_INVALID: n_ops < 1, NULL offsets / s_out, decreasing offsets, a mask with a bit at or above n_qubits; OVQE_ERR_ALLOC, with
 * the bytes needed in the text, when the store exceeds its cap (no column chunking) — the handle stays usable. */
int ovqe_subspace_matrices(ovqe_handle h, int64_t n_ops, const int64_t *offsets, const uint64_t *x, const uint64_t *z,
                           const double *coeff_re, const double *coeff_im, double *h_out_re_im, double *s_out_re_im);
/* of the last ovqe_subspace_matrices call, up to `count` entries of: [0] m [1] rows |R| [2] 1 = dense form (no lookup) [3] store bytes
 * [4] distinct x masks of the pool [5] Hamiltonian x-groups (0 when h_out was NULL) [6] expand launches [7] sigma launches [8] Gram
 * launches [9] block pairs computed [10..13] HIP-event times in microseconds: rows, expand, sigma, Gram + finish; then which path the
 * call took: [14] row slices of the Gram launch [15] rows per slice (a multiple of the 16-row staging tile: above 16 a workgroup stages
 * several tiles) [16] column blocks of 64 a lane of the sigma kernel accumulates — the instantiation that ran: 1, 2 or 4 — and [17] its
 * column groups (grid y), both 0 when no sigma kernel ran (h_out NULL or no rows) [18] workgroups in x of the sigma launch (4 rows
 * each; fewer than rows / 4: the rows are strided) [19] workgroups of the expand launch (256 store elements each; fewer than
 * rows * mb / 256: strided), 0 without rows.  Callers that ask for 14 entries see no change; zeros before the first call */
int ovqe_subspace_info(ovqe_handle h, int64_t *info, int count);

/* ---- measurement support (bench.py): average device time in ms of `reps` back-to-back launches of
 * one Pauli-rotation sweep, bracketed by HIP events on the handle's stream */
int ovqe_time_pauli_rotation(ovqe_handle h, uint64_t x, uint64_t z, double phi, int warmup, int reps,
                             double *avg_ms);
/* device time in ms of the most recent ovqe_energy_batch launch (HIP events); 0 for a call that is not timed: a lone evaluation
 * beyond the fused kernels' register sizes, small batches through the mapped buffer */
int ovqe_last_batch_ms(ovqe_handle h, double *ms);

/* amplitudes the last ovqe_pool_gradients call (which = 0) or ovqe_apply_exp_pauli_sum call (which = 1) walked instead of the
 * register ("screen_sparse"): the support of psi, resp. its closure under the operator's x-groups; -1 when the call walked the
 * register (dense state, sharded register, option off).  which = 2: determinants of the symmetry sector whose materialised
 * Hamiltonian produced sigma = H psi of the last ovqe_pool_gradients call (option "screen_sector", default 1: real Hamiltonian,
 * real psi listing at least "screen_sector_min" = 1024 amplitudes; the tables are built once per Hamiltonian on the closure of
 * psi's support under its x-groups), 0 when sigma came from the register / the tile cover.  which = 3: matrix-vector rounds
 * the last ovqe_sector_ground_state took to saturate the block of H connected to the reference determinant (the call
 * returns OVQE_ERR_STATE instead of diagonalising a truncated block when the search does not saturate).  which = 4 / 5:
 * passes over the state (kernel launches that stream the shard) of the last ovqe_apply_pauli_rotations / ovqe_bilinear /
 * ovqe_expectation call, and the bytes those passes move by construction (fused runs and tile covers make both smaller
 * than one sweep per rotation / x-group: what bench.py's `sharded` block reports next to its formula rates).  which = 6: the kernel
 * forms of the sector path that served the handle since the program was set, as bits — 0 / 1 / 2 / 3 forward sweeps on pair words /
 * 64-bit words with rounds / per-wave streams / regular supports by bit arithmetic, 4..7 the backward sweeps of
 * ovqe_energy_gradient in the same order, 8 / 9 first / second form of the pair-table builder (the tests name the geometry behind
 * every form: DESIGN.md section 4); then the choices inside a form, set where the kernel is launched — 10 / 11 the first sweep form
 * with its pair words staged two chunks ahead / not, 12 / 13 the second and third forms with their scatter indices held in LDS /
 * read late, 14 / 15 the pair-table builder on a dense slot map / by binary search (tiles of more than 16 index bits), 16 / 17
 * lambda = H psi (gradients, Lanczos) stored by LDS atomics behind a memset / by one launch per <H> sweep in sequence, 18 / 19 its
 * workgroups of 512 / 1024 threads, 20..24 the coding of the materialised <H>, one bit per outcome that at least one sweep took:
 * 24-bit packed words, 32-bit dictionary words, explicit values because the dictionary overflowed, explicit values because a sample
 * fitted a dictionary and the whole stream did not, explicit values because option "sector_dict" is 0; 25..29 / 30..34 / 35..39 the
 * workgroup sizes 64 / 128 / 256 / 512 / 1024 the circuit sweeps / the backward sweeps / the sweeps of a regular support (both
 * directions) were launched with.  which = 7: the kernel forms of the support-compacted path (programs whose reachable support
 * holds at most 4096 basis states) that served the handle since the program was set, as bits — 0 one evaluation per workgroup
 * (batches <= 256), 1 / 2 one evaluation per wave with / without its op table staged in LDS, 3 two per wave on rows of 64-bit
 * words (batches >= 2048), 4 / 5 two / four per wave without rows; 6 / 7 / 8 ovqe_energy_gradient per workgroup / per wave
 * staged / per wave; 9 a call that wanted the path was served by the other paths (no compact support, or no form fits the
 * program's LDS budget).  which = 8..13: the most recent launch of the fused whole-circuit kernel (registers up to 16 qubits) since
 * the program was set, zeros when there was none.  8: its form as bits — 0 real amplitudes, 1 state in LDS (else one global slice per
 * workgroup), 2-3 threads per workgroup (0 = 64, 1 = 256, 2 = 1024), 4 parameters and energies through the mapped buffer, 5 result
 * polled in that buffer, 6 device-resident entry point (ovqe_energy_batch_device).  9: workgroups launched (below B: a workgroup
 * takes several evaluations in turn).  10: segments of the program (runs of ops whose entries fit the LDS cos/sin table).
 * 11: chunks the terms of the general expectation entries are staged in.  12: general (x-group, pattern) entries.  13: flat
 * single-term items */
int ovqe_last_support(ovqe_handle h, int32_t which, int64_t *support);
/* shape of the compiled program (diagnostics / tests), up to `count` entries of:
 *   [0] ops of the sequential program  [1] Pauli rotations  [2] literal X/H/CNOT ops  [3] streaming sweeps per
 *   evaluation  [4] of those, LDS-tiled multi-op sweeps  [5] ops of the fused-kernel program
 *   [6] support-compacted program: -1 not analysed yet, 0 none, else the size of the reachable support
 *   [7] tile sweeps of the stored Hamiltonian's expectation (0 until first used / when not tiled)  [8] x-groups
 *   that keep their own sweep  [9] (group, pattern) entries  [10] merged terms  [11] pair x term evaluations per tile
 *   [12] 1 when streaming energies of this program keep the state as 2^n real amplitudes
 *   [13..15] support-compacted program: ops, active pairs per evaluation, entries of the restricted Hamiltonian
 *   [16..21] sector path (0 until its tables exist): support size, circuit sweeps, active pairs per evaluation, <H> sweeps
 *   (0: circuit only, <H> by the compact cover), matrix elements of the materialised Hamiltonian (padding included), table
 *   bytes  [22..24] with option "sector_profile" = 1: HIP-event time in microseconds of the circuit sweeps and of the <H>
 *   kernel of the most recent sector evaluation; bytes that kernel reads per evaluation
 *   [25] determinants of the block of H (restricted to the support) that the last ovqe_sector_ground_state diagonalised
 *   [26..27] support-compacted program: colliding lane pairs per evaluation (LDS bank conflicts of the circuit's pair
 *   rotations) with the support numbered in discovery order, and with the numbering in use (option "sparse_renumber")
 *   [28..29] sector path on a REGULAR support (the full coset of the program's Z2 symmetries, e.g. the spin-parity quarter of
 *   the register that the reference's QUCCSD templates populate; option "sector_regular", default 1): slot bits of a circuit
 *   tile — the sweeps then run from bit arithmetic, without pair words — and the number of free (dependent) index bits; 0 else
 *   [30..32] support-compacted program, batched workgroup kernel (0 when no instance of it holds the program): owner pieces of the
 *   restricted Hamiltonian that hold entries, entry slots per thread, LDS reads per thread and state of the <H> contraction
 *   [33..37] support-compacted program: LDS array cycles per evaluation by the host planner's bank model (an access of 32 lanes
 *   costs, per group of lanes it is served in, the largest number of distinct 8-byte words on one bank: reads one group of 32
 *   against 32 banks, writes two groups of 16 against 16; conflict-free: 1 and 2) — [33] the reads and [34] the writes of both
 *   amplitudes over the rows of 32 lanes of the circuit with the tables in use, [35] the slot and owner reads of the <H>
 *   contraction of the batched workgroup kernel (0 when no instance holds the program), [36] / [37] the reads / writes of the
 *   rows with the support numbered in discovery order, pairs in list order.  The rows the kernel adds to fill its pipeline
 *   (conflict-free by construction) are not counted
 *   [38..45] sector path (0 until its tables exist): index bits of a circuit tile, index bits of an <H> tile (0: circuit only), slot
 *   bits of the pair words (13, 14 or 15, decided by the widest op), amplitudes of the largest circuit tile, of the largest <H>
 *   tile, entries of the largest dictionary of an <H> sweep, dictionary entries summed over the <H> sweeps (a sweep that keeps
 *   explicit values counts 0), circuit sweeps whose tiles are taken largest first (sweeps of 512 tiles or more) */
int ovqe_program_info(ovqe_handle h, int64_t *info, int count);
/* The stored program as its sequence of Pauli rotations exp(-i (coeff[r] theta[pidx[r]] + phi0[r]) P_r), P_r = (x[r], z[r]) in
 * index-bit space, in execution order (pidx < 0: a constant angle) — for a gate program in Clifford-frame form
 * (ovqe_set_gate_program, option "clifford_frame") the rotations with their CONJUGATED strings, i.e. what the reference's
 * template list (ref:openvqe/common_files/circuit.py:13-106, executed by ref:openvqe/ucc_family/get_energy_qucc.py:47-52) becomes
 * once its Clifford gates are moved to the end; for ovqe_set_program the rotations as given.  *count receives the number of
 * rotations; up to `capacity` of them are written (arrays may be NULL when capacity is 0).  OVQE_ERR_STATE when no program is set
 * or the program still holds literal X / H / CNOT ops (a literal list, an open or forced frame).  Diagnostics / tests: lets a
 * checker evaluate the very sequence the kernels run with an independent simulator. */
int ovqe_get_rotation_program(ovqe_handle h, int64_t capacity, uint64_t *x, uint64_t *z, double *coeff, double *phi0,
                              int32_t *pidx, int64_t *count);

#ifdef __cplusplus
}
#endif
#endif /* OVQE_SV_H */
