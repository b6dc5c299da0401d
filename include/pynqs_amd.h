/*
 * pynqs_amd.h -- C ABI of libpynqs_amd.so, the MI355X (gfx950) determinant / local-energy engine.
 *
 * This is the drop-in boundary for PyNQS' `libs.C_extension` hot path.  The reference has no C ABI:
 * its boundary is a pybind11/LibTorch module (cpp_src/tensor/bind.cpp:317-391) whose functions take
 * at::Tensor.  Each entry point below names the reference interface it replaces (file:line relative
 * to the PyNQS tree); the Python shim pynqs_amd/C_extension.py re-creates the reference's Python
 * signatures on top of these calls (see INTEGRATION.md for the binding a maintainer would add).
 *
 * Conventions
 *  - Every pointer is a DEVICE pointer (HIP, same device as `stream`) unless marked [host].
 *  - ONVs are little-endian 64-bit words, `len = (sorb-1)/64 + 1` words per determinant; orbital j is
 *    bit j%64 of word j/64, even j = alpha, odd j = beta (cpp_src/tensor/cpu_tensor.cpp:8-44).
 *    The reference's uint8[n, 8*len] tensors are these words viewed as bytes.
 *  - `dtype`: PYNQS_F32 or PYNQS_F64 = element type of h1e / h2e / hmat (the reference dispatches on
 *    h1e's dtype, cpp_src/tensor/cpu_tensor.cpp:249,298).
 *  - h1e: T[sorb*sorb] row-major; h2e: T[pair*(pair+1)/2], pair = sorb*(sorb-1)/2, antisymmetrised
 *    packed triangle (cpp_src/tensor/integral.cpp:6-60).
 *  - The caller owns all buffers.  Calls enqueue work on `stream` (a hipStream_t; NULL = default
 *    stream) and return without synchronising, like the reference's CUDA path (cuda/kernel.cu:266-277).
 *  - Return value: PYNQS_OK or a negative error code; pynqs_last_error() gives a thread-local message.
 *    No exceptions cross the ABI.  n == 0 is a valid no-op.
 *  - Thread-safe and re-entrant: no global mutable state besides the thread-local error string.
 */
#ifndef PYNQS_AMD_H
#define PYNQS_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PYNQS_ABI_VERSION 1

#define PYNQS_OK 0
#define PYNQS_EINVAL (-1)  /* bad argument: sorb/nele out of range, null pointer, bad dtype        */
#define PYNQS_ELAUNCH (-2) /* HIP launch failure (message carries hipGetErrorString)               */
#define PYNQS_ELENGTH (-3) /* check_sorb: sorb needs more words than PYNQS_MAX_SORB_LEN            */
#define PYNQS_EOVERFLOW (-4) /* check_sorb: too many electrons / virtual orbitals                 */

#define PYNQS_F32 0
#define PYNQS_F64 1

/* Limits.  The reference fixes MAX_SORB_LEN at compile time (cpp_src/common/default.h:3-10); here the
 * word count is a run-time dispatch over 1..3 and the limits are those of its MAX_SORB_LEN=3 build. */
#define PYNQS_MAX_SORB_LEN 3
#define PYNQS_MAX_SORB 192
#define PYNQS_MAX_NELE 120
#define PYNQS_MAX_NVIR 120

int pynqs_abi_version(void);
const char *pynqs_last_error(void);

/* [host] cpp_src/cpu/excitation.cpp:8-16 (get_Num_SinglesDoubles): singles+doubles, identity excluded. */
int64_t pynqs_num_sd(int sorb, int noA, int noB);

/* [host] cpp_src/tensor/bind.cpp:282-301 (check_sorb): PYNQS_OK, PYNQS_ELENGTH or PYNQS_EOVERFLOW. */
int pynqs_check_sorb(int sorb, int nele);

/* cpp_src/tensor/bind.cpp:239-250 (get_comb_hij_fused) -> cpu_tensor.cpp:220-272 / cuda kernel.cu:224-277.
 * comb [nbatch][ncomb][len] (row 0 = bra itself; may be NULL to skip the write), hmat T[nbatch][ncomb]
 * (column 0 = <x|H|x>), ncomb = pynqs_num_sd()+1. */
int pynqs_comb_hij_fused(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB,
                         const void *h1e, const void *h2e, int dtype, uint64_t *comb, void *hmat,
                         void *stream);

/* cpp_src/tensor/bind.cpp:66-83 (get_comb_tensor) -> cpu_tensor.cpp:164-218.  comb as above;
 * comb_pm1 (may be NULL) = double[nbatch][ncomb][sorb], the flag_bit=True +-1 expansion (the reference
 * hard-codes double there, cpu_tensor.cpp:191-195). */
int pynqs_comb(const uint64_t *bra, int64_t nbatch, int sorb, int noA, int noB, uint64_t *comb,
               double *comb_pm1, void *stream);

/* cpp_src/tensor/bind.cpp:39-64 (get_hij_torch) -> cpu_tensor.cpp:274-325.  ket_is_3d: ket[n][m][len]
 * (local-energy mode) else ket[m][len] (full matrix).  hmat T[n][m]; excitation degree > 2 gives 0. */
int pynqs_hij(const uint64_t *bra, int64_t n, const uint64_t *ket, int64_t m, int ket_is_3d,
              const void *h1e, const void *h2e, int dtype, int sorb, int nele, void *hmat, void *stream);

/* cpp_src/tensor/bind.cpp:24-37 (onv_to_tensor) -> cpu_tensor.cpp:46-88: out T[n][sorb] = +1 / -1. */
int pynqs_onv_to_pm1(const uint64_t *bra, int64_t n, int sorb, int dtype, void *out, void *stream);

/* cpp_src/tensor/bind.cpp:9-22 (tensor_to_onv) -> cpu_tensor.cpp:8-44: occ uint8[n][sorb] (1 = occupied,
 * anything else = empty) -> out uint64[n][len]. */
int pynqs_pm01_to_onv(const uint8_t *occ, int64_t n, int sorb, uint64_t *out, void *stream);

/* cpp_src/tensor/bind.cpp:216-236 (wavefunction_lut, little_endian=True) -> cpu_tensor.cpp:589-688 /
 * cuda kernel.cu:608-680.  keys uint64[nkeys][len] sorted ascending as multi-word integers (most
 * significant word last); idx[i] = position of onv[i] or -1, mask[i] = found. */
int pynqs_wavefunction_lut(const uint64_t *keys, int64_t nkeys, const uint64_t *onv, int64_t n, int sorb,
                           int64_t *idx, uint8_t *mask, void *stream);

/* cpp_src/tensor/bind.cpp:303-314 (spin_flip_rand) -> cpu_tensor.cpp:90-137 / cuda kernel.cu:691-716: one random
 * single/double move per walker: r0 uniform on [0, nsd] (both ends), r0 == 0 keeps the walker, else excitation
 * rank r0-1 is applied.  out may alias bra (in place).  The stream is a counter-based hash of
 * (seed, offset + walker index): pass a different `offset` (e.g. a running sample count) on every call. */
int pynqs_spin_flip_rand(const uint64_t *bra, int64_t n, int sorb, int noA, int noB, uint64_t seed,
                         uint64_t offset, uint64_t *out, void *stream);

/* ---- integral plan: the fast path ---------------------------------------------------------------
 * The reference keeps h2e as one packed triangle over all spin-orbital pairs (integral.cpp:6-60); random
 * gathers from it are bound by the CU's vector L1.  A plan is a spin-blocked dense re-layout of the SAME
 * values (pynqs_amd/csrc/plan.h) in caller-owned device memory; it is built once per (h1e, h2e) and then
 * replaces the two pointers.  Needs an even sorb.  Results are bit-identical to the direct entry points.
 *   pynqs_plan_bytes : [host] size of the plan buffer in bytes, or -1 if unsupported
 *   pynqs_plan_build : fill `plan` from the reference-layout h1e / h2e (one kernel, no sync)          */
int64_t pynqs_plan_bytes(int sorb, int dtype);
int pynqs_plan_build(const void *h1e, const void *h2e, int sorb, int dtype, void *plan, void *stream);

/* get_comb_hij_fused (bind.cpp:239-250) on a plan.  Same outputs as pynqs_comb_hij_fused. */
int pynqs_comb_hij_fused_plan(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB,
                              const void *plan, int dtype, uint64_t *comb, void *hmat, void *stream);

/* ---- fused local energy (no comb / Hmat materialisation), on a plan, f64 ---------------------------
 * SAMPLE_SPACE method: vmc/energy/eloc.py:326-401 (_only_sample_space) = get_comb_hij_fused +
 * WavefunctionLUT.lookup (utils/public_function.py:817-838, cpu_tensor.cpp:589-688) + the contraction
 * eloc.py:395-396, in one pass.  keys uint64[nkeys][len] sorted as for pynqs_wavefunction_lut; wf is
 * double[nkeys] or interleaved complex double[nkeys][2]; eloc / psi0 have the same element type ([nbatch] or
 * [nbatch][2]).  psi(x') = 0 for x' outside the table; psi0 = psi(x) (0 if x itself is not in the table,
 * eloc is then inf/nan exactly like the reference's division).  The sum is taken as (sum_k H_k psi_k) / psi_0.
 * Scale: E_loc is homogeneous of degree 0 in psi, and every entry that divides by psi(x) -- the SAMPLE_SPACE entries below, their flip
 * passes and pynqs_reduce_contract -- is correct for ANY finite non-zero psi whose sums sum_k H_k psi_k are finite: the complex
 * division scales numerator and divisor by one power of two first (detcore.h: scaled_cdiv), so |psi(x)|^2 is never formed at the
 * caller's scale (it would overflow above 2^512 and lose digits below 2^-511).  Multiplying every amplitude by 2^k changes no bit of a
 * result that is added in a fixed order (the indexed form, the contraction).  psi(x) = 0 and non-finite amplitudes give a non-finite
 * E_loc, as before. */
int pynqs_eloc_sample_space(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB,
                            const void *plan, const uint64_t *keys, int64_t nkeys, const double *wf,
                            int wf_is_complex, double *eloc, double *psi0, void *stream);

/* ---- hash table over the sorted sample keys (the reference's optional GPU table: cuda/hashTable.cu,
 * cuda_tensor.cpp:489-559 hash_build / hash_lookup, off by default: utils/public_function.py:23 USE_HASH).
 * Open addressing in caller-owned memory; values are the positions in the SORTED key array, so a lookup returns
 * exactly what pynqs_wavefunction_lut returns.
 *   pynqs_hash_bytes  : [host] table size in bytes for nkeys keys
 *   pynqs_hash_build  : fill `table` from keys uint64[nkeys][len] (any order, distinct)
 *   pynqs_hash_lookup : idx[i] = position of onv[i] in the key array or -1, mask[i] = found
 *   pynqs_eloc_sample_space_hash : pynqs_eloc_sample_space with the table instead of the sorted keys        */
int64_t pynqs_hash_bytes(int64_t nkeys, int sorb);
int pynqs_hash_build(const uint64_t *keys, int64_t nkeys, int sorb, void *table, void *stream);
int pynqs_hash_lookup(const void *table, int64_t nkeys, const uint64_t *onv, int64_t n, int sorb, int64_t *idx,
                      uint8_t *mask, void *stream);
int pynqs_eloc_sample_space_hash(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB,
                                 const void *plan, const void *table, int64_t nkeys, const double *wf,
                                 int wf_is_complex, double *eloc, double *psi0, void *stream);

/* ---- spin-flip-projected SAMPLE_SPACE: vmc/energy/flip.py:322-418 (_only_sample_space_flip).
 *   E_loc(x) = [ sum_k H_k psi(x'_k) + eta * sum_k H_k eta_m(x'_k) psi(flip(x'_k)) ] / (extra_norm^2 psi(x))
 * with flip = alpha <-> beta exchange and eta_m = (-1)^(doubly occupied orbitals of x') (utils/public_function.py:966-1007).
 * The first sum / psi(x) is pynqs_eloc_sample_space[_hash]; these entries return the second one:
 *   out[x] = sum_k H_k eta_m(x'_k) psi(flip(x'_k)) / psi0[x],   psi0 = psi(x) from that call (an INPUT here),
 * one more pass of the same kernel (the filters are asked with the partner orbitals' Zobrist values).              */
int pynqs_eloc_sample_space_flip(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB,
                                 const void *plan, const uint64_t *keys, int64_t nkeys, const double *wf,
                                 int wf_is_complex, const double *psi0, double *out, void *stream);
int pynqs_eloc_sample_space_hash_flip(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB,
                                      const void *plan, const void *table, int64_t nkeys, const double *wf,
                                      int wf_is_complex, const double *psi0, double *out, void *stream);

/* ---- SAMPLE_SPACE local energy, key-major (kernels_eloc_keys.hip): the same sum as pynqs_eloc_sample_space -- vmc/energy/eloc.py:326-401,
 * psi(x') from the table of the sample space, 0 outside it -- computed by walking the TABLE: every key within a double excitation of
 * the walker (popcount(x ^ key) <= 4) contributes <x|H|key> psi(key), evaluated from the two bit patterns.  Work per walker is nkeys
 * instead of ncomb: the entry for large orbital spaces (ncomb ~ sorb^4) and for small tables.
 *   keys uint64[nkeys][len] in ANY order (no sorting, no hash table), nkeys < 2^27; wf double[nkeys] or complex double[nkeys][2].
 *   flip = 0: eloc[x] = sum / psi(x), psi0[x] (OUTPUT) = psi(x) = the table value of the key equal to x, 0 if there is none;
 *   flip = 1: the projected form's partner sum (flip.py:322-418): eloc[x] = sum_x' <x|H|x'> eta_m(x') psi(flip x') / psi0[x], psi0 INPUT. */
int pynqs_eloc_sample_space_keys(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const void *plan,
                                 const uint64_t *keys, int64_t nkeys, const double *wf, int wf_is_complex, int flip, double *eloc,
                                 double *psi0, void *stream);

/* ---- the same behind a BLOCK INDEX of the keys (round 3; kernels_keys_index.hip, kernels_eloc_keys.hip INDEXED): the sorb bits are cut
 * into 5 blocks; a determinant within a double excitation of x agrees with x in at least one whole block, so only the keys that share a
 * block value with the walker are loaded and compared (binary searches in the per-block sorted lists), each counted in the first block it
 * agrees in.  Work per walker ~ the number of such keys (tens for a table of samples at sorb >= 56) instead of nkeys.
 *   pynqs_keys_index_bytes     : [host] size of the index (60 bytes per key), -1 on bad arguments (sorb even, nkeys < 2^27)
 *   pynqs_keys_index_workspace : [host] scratch bytes for the build
 *   pynqs_keys_index_build     : index <- keys uint64[nkeys][len] (any order, distinct); five stable radix sorts: the index, and
 *                                with it the order of the kernel's additions, is a function of the key array alone
 *   pynqs_keys_index_density   : *sum_sq (device, uint64) = sum over the runs of equal block values of length^2: a key of the table used
 *                                as a walker meets sum_sq / nkeys keys through the index (streamed: nkeys).  CAS-like tables share blocks
 *                                among thousands of keys (Fe2S2: 21.5e3 per walker of 18.5e3 keys) -- the streamed or the column-major
 *                                form is the one to use there; tables of samples at sorb >= 56 do not (13 of 65.5e3 at sorb 120 / 184)
 *   pynqs_eloc_sample_space_indexed : pynqs_eloc_sample_space_keys with the index (same arguments, same results up to the order
 *                                of the additions; no atomics: bit-reproducible)                                                          */
int64_t pynqs_keys_index_bytes(int64_t nkeys, int sorb);
int64_t pynqs_keys_index_workspace(int64_t nkeys, int sorb);
int pynqs_keys_index_build(const uint64_t *keys, int64_t nkeys, int sorb, void *index, void *workspace, void *stream);
int pynqs_keys_index_density(const void *index, int64_t nkeys, int sorb, uint64_t *sum_sq, void *stream);
int pynqs_eloc_sample_space_indexed(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const void *plan,
                                    const uint64_t *keys, int64_t nkeys, const void *index, const double *wf, int wf_is_complex,
                                    int flip, double *eloc, double *psi0, void *stream);

/* [host] the form a SAMPLE_SPACE launch takes, from the very rule the launch uses (0 on success, PYNQS_EINVAL on bad arguments; nbatch >= 1).
 *   pynqs_eloc_sample_space_form : the column-major entry points (hash = 0: pynqs_eloc_sample_space / _flip on sorted keys, hash = 1:
 *       the _hash forms on a table of nkeys keys).  out = {kind, two_level, block, sweep, pre, lds_bytes, nchunks, chunk_len}:
 *       kind 0 = sorted-key search, 1 = hash table without filters, 2 = the filtered kernel; two_level = second-level filter in use;
 *       block = threads per workgroup; sweep = block sweeps (else rank-by-rank scan); pre = string prefilter; lds_bytes = dynamic LDS;
 *       nchunks / chunk_len = workgroups per walker and columns per workgroup.
 *   pynqs_eloc_sample_space_keys_form : pynqs_eloc_sample_space_keys (indexed = 0) / _indexed (indexed = 1).
 *       out = {groups, nchunks, chunk_len}: workgroups along the walkers, chunks of the key array per group, keys per chunk. */
int pynqs_eloc_sample_space_form(int64_t nbatch, int sorb, int nele, int noA, int noB, int64_t nkeys, int hash, int64_t out[8]);
int pynqs_eloc_sample_space_keys_form(int64_t nbatch, int sorb, int64_t nkeys, int indexed, int64_t out[3]);

/* ---- duplicates among determinants, without a sort (`Func`, vmc/energy/flip.py:44-50: torch.unique(dim=0,
 * return_inverse=True) on the x' that reach the ansatz).  first[i] = smallest j with onv[j] == onv[i] (int32[n]);
 * the rows with first[i] == i are the distinct determinants in order of first appearance.  Deterministic.
 *   pynqs_unique_workspace : [host] bytes of scratch for n rows (-1: n out of range, n < 2^30)             */
int64_t pynqs_unique_workspace(int64_t n);
int pynqs_unique_first(const uint64_t *onv, int64_t n, int sorb, void *workspace, int32_t *first, void *stream);

/* ---- SIMPLE method with a real RBM amplitude, fully fused, f64 -------------------------------------------
 * vmc/energy/eloc.py:121-203 (_simple: get_comb_hij_fused + ansatz on all nbatch*ncomb kets + contraction) for
 * the reference's RBMWavefunction with rbm_type "real" (vmc/ansatz/rbm/rbm.py:186-211):
 *   psi(x) = exp(visible_bias . x) * prod_h 2 cosh(hidden_bias[h] + sum_o weights[h][o] x_o),  x_o = +1 / -1.
 * The parameters are re-laid out once per parameter update into a caller-owned "RBM table" (pynqs_amd/csrc/rbm.h):
 *   pynqs_eloc_rbm_supported : [host] 1 if exp(+-4 W) of all (orbital, hidden unit) pairs of this problem fits the
 *                           CU's LDS next to the walker tables (the kernel's working set), else 0
 *   pynqs_rbm_table_bytes : [host] size of the table in bytes, or -1 for bad sizes
 *   pynqs_rbm_table_build : weights double[nhidden][sorb] (row-major, the reference's parameter shape),
 *                           hidden_bias double[nhidden], visible_bias double[sorb] or NULL (= 0)
 *   pynqs_eloc_rbm        : eloc[nbatch] = sum_x' <x|H|x'> psi(x')/psi(x) over x' = x and all singles/doubles;
 *                           psi (may be NULL) receives psi(x).  The amplitude ratios are evaluated from the
 *                           2 or 4 flipped orbitals (no overflow for any theta); results agree with the
 *                           materialised path to rounding (tests: 1e-8 Ha). */
int pynqs_eloc_rbm_supported(int sorb, int nele, int noA, int noB, int nhidden);
/* [host] the form a launch of pynqs_eloc_rbm / _flavour (green = 0) or pynqs_green_rbm (green = 1) on nbatch walkers takes, from the
 * very rule the launch uses: -1 if unsupported, else bit 0 = the windowed kernel (sorb x nhidden beyond the LDS), bit 1 = a walker's
 * tiles are cut over several workgroups that add their parts with atomics (fewer than 1024 walkers). */
int pynqs_eloc_rbm_form(int64_t nbatch, int sorb, int nele, int noA, int noB, int nhidden, int green);
/* [host] the whole launch behind that form, and behind pynqs_eloc_jrbm (jastrow = 1, green = 0) and pynqs_green_jrbm (jastrow = 1,
 * green = 1; their signed and flip passes launch alike): out6[0] = workgroups, [1] = threads per workgroup, [2] = bytes of dynamic LDS,
 * [3] = hidden units resident in LDS, [4] = workgroups per walker, [5] = 1 if the walker's Jastrow pair factors are kept in LDS.
 * Returns 0, or -1 (out6 untouched) where the launch is not served or nbatch is outside [1, 2^31 - 1]. */
int pynqs_eloc_rbm_geometry(int64_t nbatch, int sorb, int nele, int noA, int noB, int nhidden, int green, int jastrow, int64_t *out6);
int64_t pynqs_rbm_table_bytes(int sorb, int nhidden);
int pynqs_rbm_table_build(const double *weights, const double *hidden_bias, const double *visible_bias, int sorb,
                          int nhidden, void *table, void *stream);
int pynqs_eloc_rbm(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const void *plan,
                   const void *rbm_table, int nhidden, double *eloc, double *psi, void *stream);
/* The reference's other RBM amplitudes that share the hidden-unit product (rbm.py:199-211), from the same table:
 *   PYNQS_RBM_REAL  psi = exp(a.x)  prod_h 2cosh(theta_h)                    eloc, psi double[nbatch]  (= pynqs_eloc_rbm)
 *   PYNQS_RBM_TANH  psi = tanh(a.x) prod_h 2cosh(theta_h)   (rbm_type "tanh") eloc, psi double[nbatch]
 *   PYNQS_RBM_PHASE psi = exp(i (a.x + sum_h ln 2cosh(theta_h)))  ("pRBM")   eloc, psi double[nbatch][2] = (re, im)
 * ("cos" and "complex" are not fused: they run through the module path of pynqs_amd.energy.local_energy.) */
#define PYNQS_RBM_REAL 0
#define PYNQS_RBM_TANH 1
#define PYNQS_RBM_PHASE 2
int pynqs_eloc_rbm_flavour(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const void *plan,
                           const void *rbm_table, int nhidden, int flavour, double *eloc, double *psi, void *stream);

/* ---- the spin-flip-projected SIMPLE local energy (vmc/energy/flip.py, _simple_flip) of the three flavours above, fused ----------------
 *   E_proj(x) = sum_k <x|H|x'_k> [psi(x'_k) + eta eta_m(x'_k) psi(flip x'_k)] / psi(x) / extra_norm^2
 * flip exchanges the orbitals 2k <-> 2k+1, eta_m(y) = (-1)^(number of doubly occupied spatial orbitals of y), eta = +-1 the projection.
 * THE MIRRORED TABLE: psi(flip y) of the parameters (W, a, b) is psi(y) of (Wm, am, b) with Wm[h][o] = W[h][o^1], am[o] = a[o^1]
 * (for the Jastrow factor Mm[i][j] = M[i^1][j^1]): a second table, built by pynqs_rbm_table_build (pynqs_jastrow_table_build) from the
 * mirrored parameters, on the same walkers and the same excitations.  With psim the amplitude of the mirrored table,
 *   R(x) = psim(x) / psi(x),   E(x) = sum_k h_k psi(x'_k) / psi(x),   Em(x) = sum_k sigma_k h_k psim(x'_k) / psim(x),
 *   E_proj(x) = [E(x) + eta eta_m(x) R(x) Em(x)] / extra_norm^2,      sigma_k = eta_m(x'_k) eta_m(x) = (-1)^pi_k,
 *   pi_k = XOR over the flipped orbitals o of x'_k of the walker's bit at o^1, XOR the number of spatial orbitals with both spin orbitals
 *   flipped (the diagonal column: sigma = +1).  No spin symmetry of the integrals is assumed (Em is NOT E of the flipped walker).
 *   pynqs_eloc_rbm_signed : pynqs_eloc_rbm_flavour with every column's matrix element times sigma_k: called with the MIRRORED table it
 *                           returns eloc = Em and psi = psim (same shapes, psi may be NULL); with any table, that table's signed sum.
 *   pynqs_eloc_rbm_flip   : eloc = E_proj, psi = psi(x) (required).  rbm_table_mirror: the mirrored table.  extra_norm_dev: DEVICE pointer
 *                           to extra_norm, or NULL to take the value `extra_norm`.  work: 2 nbatch doubles (PYNQS_RBM_PHASE: 4 nbatch) of
 *                           device scratch; on return work[0 .. ) = Em and behind it psim, in eloc's / psi's layout.  Three launches on
 *                           `stream` (the plain pass, the signed pass, a combine kernel that forms R and eta_m(x) from the walker's bits,
 *                           in complex arithmetic for PYNQS_RBM_PHASE); no host read-back or synchronisation.
 *   pynqs_eloc_rbm_flip_supported / _form : [host] as pynqs_eloc_rbm_supported / pynqs_eloc_rbm_form(green = 0); both passes (and
 *                           pynqs_eloc_rbm_signed) take the form of the plain launch. */
int pynqs_eloc_rbm_flip_supported(int sorb, int nele, int noA, int noB, int nhidden);
int pynqs_eloc_rbm_flip_form(int64_t nbatch, int sorb, int nele, int noA, int noB, int nhidden);
int pynqs_eloc_rbm_signed(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const void *plan,
                          const void *rbm_table, int nhidden, int flavour, double *eloc, double *psi, void *stream);
int pynqs_eloc_rbm_flip(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const void *plan,
                        const void *rbm_table, const void *rbm_table_mirror, int nhidden, int flavour, double eta, double extra_norm,
                        const double *extra_norm_dev, double *eloc, double *psi, double *work, void *stream);

/* ---- SIMPLE method with an RBM with COMPLEX parameters, fully fused (kernels_rbm_complex.hip) -----------------------------
 * psi(x) = exp(a.x) prod_h 2 cosh(b_h + sum_o W[h][o] x_o) with complex a, b, W: rbm.py:199-211, rbm_type "complex"
 * (weights double[nhidden][sorb][2], hidden_bias double[nhidden][2], visible_bias double[sorb][2] or NULL: the reference's
 * params_weights / params_hidden_bias / params_visible_bias, (re, im) pairs).  rbm_type "cos" (prod_h cos(theta_h), real
 * parameters) is the same function of i*W, i*b up to the constant 2^nhidden: pass log_scale = nhidden * ln 2.
 *   pynqs_eloc_crbm_supported : [host] 1 if the complex rows of all (orbital, hidden unit) pairs fit the CU's LDS
 *   pynqs_crbm_table_bytes / _build : re-laid-out parameters in caller-owned memory (rebuild after every update)
 *   pynqs_eloc_crbm : eloc double[nbatch][2] = sum_x' <x|H|x'> psi(x')/psi(x);  psi double[nbatch][2] (may be NULL) =
 *                     psi(x) exp(-log_scale). */
int pynqs_eloc_crbm_supported(int sorb, int nele, int noA, int noB, int nhidden);
/* [host] as pynqs_eloc_rbm_form, for pynqs_eloc_crbm */
int pynqs_eloc_crbm_form(int64_t nbatch, int sorb, int nele, int noA, int noB, int nhidden);
int64_t pynqs_crbm_table_bytes(int sorb, int nhidden);
int pynqs_crbm_table_build(const double *weights, const double *hidden_bias, const double *visible_bias, int sorb, int nhidden,
                           void *table, void *stream);
int pynqs_eloc_crbm(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const void *plan,
                    const void *crbm_table, int nhidden, double log_scale, double *eloc, double *psi, void *stream);

/* ---- SIMPLE method, energy gradient and amplitudes of a real RBM times a two-body Jastrow factor (kernels_rbm.hip JASTROW,
 * kernels_jastrow.hip, kernels_rbm_forward.hip) ------------------------------------------------------------------------------------
 *   psi(x) = exp(visible_bias . x + x^T M x) * prod_h 2 cosh(hidden_bias[h] + sum_o weights[h][o] x_o),  x_o = +1 / -1:
 * the reference's Jastrow (vmc/ansatz/rbm/rbm_other.py, exp(sum_ij M_ij x_i x_j), prod_dim = 1) multiplied onto its RBMWavefunction with
 * rbm_type "real" (vmc/ansatz/hybrid/multi.py).  jastrow = M: double[sorb][sorb] row-major, any real matrix (not symmetric, diagonal
 * allowed).  With S = M + M^T without its diagonal, x^T M x = tr M + sum_{i<j} S_ij x_i x_j, and flipping the orbitals F of an excitation
 * changes it by  -2 sum_{i in F} x_i r_i + 4 sum_{i<j in F} S_ij x_i x_j,  r_i = sum_j S_ij x_j:  a per-orbital factor that joins the RBM
 * kernel's per-walker table, and one (single) or six (double) pair factors exp(+-4 S_ij) read from the "Jastrow table".
 *   pynqs_jastrow_table_bytes : [host] size of the table in bytes (pynqs_amd/csrc/rbm.h: S, exp(+4 S), exp(-4 S), tr M), -1 for a bad sorb
 *   pynqs_jastrow_table_build : M -> the table, in caller-owned memory; rebuild after every parameter update (one small kernel)
 *   pynqs_eloc_jrbm_supported : [host] 1 if pynqs_eloc_jrbm serves this problem: the resident form of pynqs_eloc_rbm (sorb x nhidden
 *                               within the LDS).  There is no windowed form: 0 beyond it, and callers evaluate the module instead.
 *   pynqs_eloc_jrbm_form      : [host] as pynqs_eloc_rbm_form: -1 if unsupported, else bit 1 = a walker's tiles are cut over several
 *                               workgroups that add their parts with atomics (bit 0, the windowed kernel, is never set), bit 2 = the
 *                               walker's pair factors are kept as a triangle in LDS (4 sorb (sorb - 1) bytes; where that would cost a
 *                               workgroup per CU, and beyond 128 orbitals, they are read from the table in L2)
 *   pynqs_eloc_jrbm           : as pynqs_eloc_rbm, same outputs and conventions; rbm_table from pynqs_rbm_table_build, jastrow_table from
 *                               pynqs_jastrow_table_build.  psi (may be NULL) receives psi(x) including exp(tr M).
 *   pynqs_jrbm_forward        : psi double[n] on a list of packed determinants from scratch, as pynqs_rbm_forward (one lane per
 *                               determinant, nothing but the result written); visible_bias may be NULL.
 *   pynqs_jastrow_grad        : the estimator of pynqs_rbm_grad for M (real parameters): d ln psi / d M_ij = x_i x_j, so
 *                                 grad_jastrow[i][j] = 2 sum_n f_n x_i(n) x_j(n),  f_n = p_n (E_loc,n - <E> c_n)   (double[sorb][sorb], overwritten),
 *                                 loss (may be NULL) = 2 sum_n f_n x_n^T M x_n: the Jastrow part of the loss, to be added to pynqs_rbm_grad's.
 *                               prob, eloc double[n]; e_total: DEVICE pointer to <E>; pow: c_n double[n] or NULL for 1.  The gradients of
 *                               weights and biases do not depend on M: they come from pynqs_rbm_grad, called as for the plain RBM.
 *                               workspace: pynqs_jastrow_grad_workspace(n, sorb) bytes.  Sums run in a fixed order, no atomics: two calls
 *                               give the same bits. */
int64_t pynqs_jastrow_table_bytes(int sorb);
int pynqs_jastrow_table_build(const double *jastrow, int sorb, void *table, void *stream);
int pynqs_eloc_jrbm_supported(int sorb, int nele, int noA, int noB, int nhidden);
int pynqs_eloc_jrbm_form(int64_t nbatch, int sorb, int nele, int noA, int noB, int nhidden);
int pynqs_eloc_jrbm(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const void *plan,
                    const void *rbm_table, const void *jastrow_table, int nhidden, double *eloc, double *psi, void *stream);
/* The spin-flip-projected form for the Jastrow-RBM: pynqs_eloc_rbm_signed / _flip (formula and mirrored-table convention there) with the
 * Jastrow table and its mirror (built from Mm[i][j] = M[i^1][j^1]); served where pynqs_eloc_jrbm is; work: 2 nbatch doubles. */
int pynqs_eloc_jrbm_flip_supported(int sorb, int nele, int noA, int noB, int nhidden);
int pynqs_eloc_jrbm_flip_form(int64_t nbatch, int sorb, int nele, int noA, int noB, int nhidden);
int pynqs_eloc_jrbm_signed(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const void *plan,
                           const void *rbm_table, const void *jastrow_table, int nhidden, double *eloc, double *psi, void *stream);
int pynqs_eloc_jrbm_flip(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const void *plan,
                         const void *rbm_table, const void *jastrow_table, const void *rbm_table_mirror, const void *jastrow_table_mirror,
                         int nhidden, double eta, double extra_norm, const double *extra_norm_dev, double *eloc, double *psi, double *work,
                         void *stream);
int pynqs_jrbm_forward(const uint64_t *onv, int64_t n, int sorb, const double *weights, const double *hidden_bias,
                       const double *visible_bias, const double *jastrow, int nhidden, double *psi, void *stream);
int64_t pynqs_jastrow_grad_workspace(int64_t n, int sorb);
int pynqs_jastrow_grad(const uint64_t *onv, int64_t n, int sorb, const double *jastrow, const double *prob, const double *eloc,
                       const double *e_total, const double *pow, double *grad_jastrow, double *loss, void *workspace, void *stream);
/* ---- the Jastrow factor on the DISTINCT x' of a REDUCE front end, from their parents (kernels_jastrow_children.hip): the second, streaming
 * pass behind pynqs_rbm_forward_children (flavour PYNQS_RBM_REAL), which is neither changed nor aware of it.  Row r of the distinct list is
 * walker p = parent[r] with the orbitals F flipped, and with q0[p] = x_p^T M x_p = tr M + 1/2 sum_o x_o r_o, r_o = sum_j S_oj x_j (S from the
 * Jastrow table),
 *     psi_JRBM(x'_r) = psi_RBM(x'_r) exp(q0[p] + Delta_r),   Delta_r = -2 sum_{i in F} x_i r_i + 4 sum_{i<j in F} S_ij x_i x_j   (x: the parent's).
 *   pynqs_jastrow_children_table_bytes : [host] nwalkers x (sorb + 1) doubles (r_o for o < sorb, then q0, per parent); -1 on bad arguments
 *   pynqs_jastrow_children_prepare     : table <- r and q0 of the parents (jastrow_table: pynqs_jastrow_table_build's).  Sums run in a fixed
 *                                        order (fma chains over the orbitals ascending from 0), no atomics: two calls give the same bits.
 *   pynqs_jastrow_children_apply       : psi[r] *= exp(q0[p] + Delta_r) for r < min(*count_dev, n) (count_dev may be NULL: all n rows); psi
 *                                        double[n] as pynqs_rbm_forward_children left it.  F = onv[r] XOR walkers[p] (bits at and above
 *                                        sorb ignored); the exponent is one sum, one exp per row; no flip: Delta = 0 exactly.  Rows at and
 *                                        past the count are neither read nor written.  One thread per row, THE GRID IS NOT CAPPED (ceil(n /
 *                                        256) workgroups, no stride loop), hence no geometry entry.
 * Strangers, the contract of pynqs_rbm_forward_children's: a row whose parent is outside [0, nwalkers) or that differs from the named
 * parent in more than four orbitals gets its exponent from scratch on its own bits, tr M + sum_{i<j} S_ij x'_i x'_j; it is never truncated
 * to four flips and never clamped to walker 0.
 * Limits: sorb <= 192 (the Jastrow table's), one to three words; the hidden layer is not seen.
 * Range: the product is formed in double.  Where psi_RBM(x') and the product are both finite non-zero doubles the row obeys
 *   |psi / psi_exact - 1| <= 2^-53 [(sorb + nhidden + 16) cond(x') + (2 sorb + 4) sum_ij |M_ij| + 2 (sorb + 3) sum_{o in F} R_o
 *                                   + 28 sum_{i<j in F} |S_ij| + 16],   R_o = sum_j |S_oj|   (tests/jchildren_exact.py counts the roundings;
 * a stranger: the first two terms + 16).  A row whose RBM amplitude alone is inf, 0 or nan stays so (it is not written): pynqs_jrbm_forward
 * joins the exponents before the exponential and remains the route for such models. */
int64_t pynqs_jastrow_children_table_bytes(int64_t nwalkers, int sorb);
int pynqs_jastrow_children_prepare(const uint64_t *walkers, int64_t nwalkers, int sorb, const void *jastrow_table, void *table,
                                   void *stream);
int pynqs_jastrow_children_apply(const uint64_t *onv, int64_t n, const int32_t *count_dev, const int32_t *parent, const uint64_t *walkers,
                                 int64_t nwalkers, const void *table, const void *jastrow_table, int sorb, double *psi, void *stream);

/* ---- Green's-function Monte-Carlo move: gfmc/walker.py:260-279 (sample_update) in one kernel ---------------
 * green double[n][ncomb] (the fixed-node Green's function row of each walker, >= 0), rand_num double[n] in [0, 1),
 * comb uint64[n][ncomb][len] (get_comb_hij_fused's first output).  Per walker: beta = sum_k green[k];
 * index = first k with (green[0] + ... + green[k]) >= rand_num * beta  (the reference's
 * searchsorted(cumsum / beta, rand_num, right=False), clamped to ncomb - 1); x_new = comb[index].
 * The sums run in float64 in the kernel's own order, so the law is stated on the exact row.  G = green[x] >= 0 with m = ncomb columns,
 * S = sum G, C_k = G_0 + ... + G_k in exact arithmetic, C_{-1} = 0, u = rand_num[x], tau = m 2^-52 S:
 *   index = k only if  C_{k-1} - tau < u S <= C_k + tau  AND  (G_k > 0 or k = 0):  a column without weight is never chosen -- in fixed-node
 *     GFMC it is a move across the node -- although the bracket alone would admit it (C_{k-1} = C_k there).  u = 0 with G_0 = 0 may
 *     give index 0 or the first column with weight; the kernel gives index 0, as the reference's searchsorted does (the walker stays).
 *     A uniform farther than tau from every C_j leaves exactly one column, the exact one.
 *   A row with S = 0 gives index 0, beta = 0 and x_new = comb[0] (the rank form: bra[x]).
 *   |beta - S| <= (m - 1) 2^-53 S; equal rows give bit-equal beta, and pynqs_gfmc_sample and pynqs_gfmc_sample_rank give the same bits.
 * tau: every running sum the kernel compares is a float64 sum of at most m non-negative entries in some order, within (m - 1) 2^-53 S of
 * its exact value; so is beta, and u * beta adds one rounding; two such quantities are compared.
 * n = 0 returns PYNQS_OK and writes nothing.  (tests/gfmc_exact.py holds the law in exact integer arithmetic.) */
int pynqs_gfmc_sample(const double *green, int64_t n, int64_t ncomb, const double *rand_num, const uint64_t *comb,
                      int sorb, int64_t *index, double *beta, uint64_t *x_new, void *stream);

/* ---- the whole Green's-function row of gfmc/walker.py:167-235 (_calculate_green_kernel) in ONE kernel for a trial function
 * that is an RBM with real parameters (flavour PYNQS_RBM_REAL or PYNQS_RBM_TANH; the complex-valued phase flavour has no fixed node):
 *   r_k = psi(x'_k)/psi(x), h_k = <x|H|x'_k>;  for k >= 1: green[k] = -h_k r_k if h_k r_k < 0 (sign-preserving move) else 0;
 *   v_sf = sum of the other h_k r_k (sign-flip potential);  green[0] = max(0, lambda - h_0 - v_sf), clamped[x] = 1 if that was < 0;
 *   eloc[x] = sum_k h_k r_k (unchanged by the fixed-node construction), psi (may be NULL) = psi(x).
 * green double[nbatch][ncomb] in the reference's column order; neither comb nor the amplitude batch is materialised.
 *   pynqs_gfmc_sample_rank : pynqs_gfmc_sample for such a row: x_new = the excitation of rank index - 1 of bra[x] (index 0: bra[x]). */
int pynqs_green_rbm(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const void *plan,
                    const void *rbm_table, int nhidden, int flavour, double lambda, double *eloc, double *psi, double *green,
                    uint8_t *clamped, void *stream);
int pynqs_gfmc_sample_rank(const double *green, int64_t n, const double *rand_num, const uint64_t *bra, int sorb, int nele,
                           int noA, int noB, int64_t *index, double *beta, uint64_t *x_new, void *stream);
/* The same row for a trial function that is a real RBM times a two-body Jastrow factor, psi(x) = exp(a.x + x^T M x) prod_h 2cosh(theta_h)
 * (pynqs_eloc_jrbm's amplitude: rbm_table from pynqs_rbm_table_build, jastrow_table from pynqs_jastrow_table_build), in ONE kernel
 * (kernels_rbm.hip, GREEN and JASTROW together).  Row layout, column order, v_sf, the clamping of green[0], clamped, eloc and psi (may be
 * NULL; includes exp(tr M)) are those of pynqs_green_rbm with flavour PYNQS_RBM_REAL; pynqs_gfmc_sample_rank moves by such a row.
 * Serves what pynqs_eloc_jrbm serves: PYNQS_EINVAL where pynqs_eloc_jrbm_supported is 0 (nothing is launched) or where jastrow_table,
 * green or clamped is NULL.  The form is always "resident, one workgroup per walker" (the row finishes its diagonal in the kernel);
 * the pair factors are read from the walker's triangle in LDS or from the table in L2 exactly where bit 2 of pynqs_eloc_jrbm_form says
 * so (PYNQS_JRBM_PAIRS=lds / l2 honoured). */
int pynqs_green_jrbm(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const void *plan,
                     const void *rbm_table, const void *jastrow_table, int nhidden, double lambda, double *eloc, double *psi,
                     double *green, uint8_t *clamped, void *stream);

/* ---- statistics: utils/stats/dist_stats.py:18-79 needs sum p O, sum p |O|^2 (and sum p) before its all-reduce -----
 *   pynqs_moments_workspace : [host] bytes of the workspace (device memory, ZERO it once before the first call)
 *   pynqs_weighted_moments  : workspace[0..3] (doubles) = sum_i p_i Re x_i, sum_i p_i Im x_i, sum_i p_i |x_i|^2,
 *                             sum_i p_i; x is double[n] or interleaved complex double[n][2]; fixed order of additions. */
int64_t pynqs_moments_workspace(void);
/* closing arithmetic of dist_stats.py:59-79 on the summed moments of all ranks (moments[0..3] as above, SUMMED over
 * the ranks; inv_world = 1 / world_size as in comm.py:62-67): out5 = mean_re, mean_im, var, sd, se = sd / sqrt(counts). */
int pynqs_stats_finish(const double *moments, double inv_world, double counts, double *out5, void *stream);
int pynqs_weighted_moments(const double *x, int is_complex, const double *prob, int64_t n, void *workspace, void *stream);
/* pynqs_weighted_moments followed by pynqs_stats_finish on workspace[0..3] in ONE launch, for a single rank (no all-reduce in between):
 * the workgroup that finishes last does the closing arithmetic on the sums it has just formed.  workspace[0..3] and out5 hold bit for bit
 * what the two calls leave. */
int pynqs_weighted_moments_finish(const double *x, int is_complex, const double *prob, int64_t n, void *workspace, double inv_world,
                                  double counts, double *out5, void *stream);
/* Two forms compute these sums, with the same additions in the same order (the same bits in workspace and out5): several workgroups and
 * a ticket for the last one to finish, or -- for n <= pynqs_moments_onegroup_max() [host], where it is the faster one -- ONE workgroup
 * that needs neither ticket nor fence.  The two entry points above choose by n; this one takes the form per call (PYNQS_MOMENTS_ONEGROUP
 * runs up to n = 32768) and is pynqs_weighted_moments for out5 == NULL, pynqs_weighted_moments_finish otherwise. */
#define PYNQS_MOMENTS_AUTO 0
#define PYNQS_MOMENTS_BLOCKS 1
#define PYNQS_MOMENTS_ONEGROUP 2
int64_t pynqs_moments_onegroup_max(void);
int pynqs_weighted_moments_form(const double *x, int is_complex, const double *prob, int64_t n, void *workspace, double inv_world,
                                double counts, double *out5, int form, void *stream);

/* REDUCE method front end: vmc/energy/eloc.py:205-324 with eps_sample == 0 keeps the columns with
 * |<x|H|x'>| >= eps (eloc.py:297-298; column 0 is treated like any other).  Two passes, nothing materialised, no
 * atomics.  A walker's row is visited in tiles; T = pynqs_reduce_tiles(...) tiles per walker:
 *   pynqs_reduce_tiles : [host] T for this batch size and system (-1 on bad arguments)
 *   pynqs_reduce_count : tile_counts uint32[nbatch][T] = kept columns per tile (0 for unused tiles)
 *   pynqs_reduce_emit  : tile_offsets int64[nbatch][T] = exclusive prefix sum of tile_counts over the whole flattened
 *                        array (caller) -> kept_col int32[total], kept_onv uint64[total][len], kept_h T[total].
 *                        Walker w's records are the contiguous range that its tiles span; inside it they come tile by
 *                        tile in a reproducible order (diagonal, singles, doubles), NOT in ascending column order --
 *                        kept_col names the column of each record. */
int64_t pynqs_reduce_tiles(int64_t nbatch, int sorb, int nele, int noA, int noB);
int pynqs_reduce_count(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB,
                       const void *plan, int dtype, double eps, uint32_t *tile_counts, void *stream);
int pynqs_reduce_emit(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB,
                      const void *plan, int dtype, double eps, const int64_t *tile_offsets, int32_t *kept_col,
                      uint64_t *kept_onv, void *kept_h, void *stream);

/* Semi-stochastic REDUCE (eloc.py:257-296, eps_sample > 0; the Fe2S2 example uses eps = 1e-2, eps_sample = 1000):
 * columns with |H| >= eps are kept (the three calls above); from the others N columns are drawn with replacement,
 * p_m = |H_m| / S, and a column drawn c times carries the weight (c / N) sign(H_m) S.  The multinomial is drawn
 * hierarchically -- over the tiles on the host, inside a tile on the GPU -- which is the same distribution:
 *   pynqs_reduce_count_sums : like pynqs_reduce_count, plus tile_sums double[nbatch][T] = sum of the sub-eps |H| per
 *                             tile (eps = +inf: nothing is kept, every column can be drawn)
 *   pynqs_reduce_sample     : tile_draws int32[nbatch][T] = draws per tile (host: multinomial over tile_sums),
 *                             sample_offsets int64[nbatch][T] = exclusive prefix of tile_draws over the flattened
 *                             array, walker_scale double[nbatch] = S / N, seed for the counter-based generator.
 *                             Tile t writes one record per DISTINCT drawn column into s_col / s_onv / s_h starting at
 *                             sample_offsets[t] (at most tile_draws[t] of them; pre-fill s_col with -1 to tell the
 *                             unused slots): s_h = sign(H) * hits * walker_scale. */
int pynqs_reduce_count_sums(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB,
                            const void *plan, int dtype, double eps, uint32_t *tile_counts, double *tile_sums,
                            void *stream);
int pynqs_reduce_sample(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const void *plan,
                        int dtype, double eps, const int32_t *tile_draws, const int64_t *sample_offsets,
                        const double *walker_scale, uint64_t seed, int32_t *s_col, uint64_t *s_onv, void *s_h,
                        void *stream);

/* ---- REDUCE front end in ONE launch (kernels_reduce_onepass.hip): vmc/energy/eloc.py:205-324 (_reduce_psi) + `Func`
 * (vmc/energy/flip.py:29-63) + onv_to_tensor, i.e. everything between the walkers and the ansatz' forward:
 *   - every column of a walker's row is enumerated once; |<x|H|x'>| >= eps is kept (eloc.py:297-298, 258-262);
 *   - eps_sample > 0 (eloc.py:263-296): the sub-eps |H| are summed per tile in LDS, the N = eps_sample draws of
 *     torch.multinomial are drawn over the tiles inside the kernel (counter-based generator, `seed`), and only the tiles
 *     that received draws are enumerated a second time for the draws inside them; a column drawn c times carries the
 *     weight (c / N) sign(H) S, S = sum of the row's sub-eps |H| (the same distribution as the reference's);
 *   - every record's x' is looked up in the wave-function table (if one is given) and otherwise inserted into a
 *     de-duplication hash table in the same pass; the first occurrence of a determinant gets the next row of the
 *     DISTINCT list and writes its +1/-1 row (the ansatz' input, onv_to_tensor's layout) there.
 * No host round trip: output space is a fixed-capacity segment per (walker, chunk) -- `fixed` slots with a fixed
 * position per column for column 0, the singles and the unpaired doubles (slot = -1 in rec_col when not kept), then the
 * kept doubles compacted in tile order (decoupled look-back in LDS, reproducible), then N slots per walker for the draws.
 * Capacities are the caller's; what was NEEDED comes back in seg_count / counters, so that an overflow is detected (and
 * the call repeated with larger buffers) without anything having been read back in between.
 *
 *   pynqs_reduce_onepass_plan     : [host] what the launch will decide for a system, a batch and the caller's limits; what to allocate
 *   pynqs_reduce_onepass_list_capacity : [host] the largest io->cap_doubles with which pynqs_reduce_onepass keeps a segment's
 *                                   records in an LDS list -- its LIST form (one list per segment) or, without draws, the flushing
 *                                   form (the list is emptied as it fills: 2^30 - 1 = any capacity on rows of more than 65536
 *                                   columns and whenever there is no de-duplication table, else a tenth of a segment's columns);
 *                                   -1: never.  Beyond it the look-back form runs, which long rows should avoid (the multi-pass entry
 *                                   points pynqs_reduce_count / _emit are 2-4 x faster there).  with_row_cache / without_table: whether
 *                                   io->row_cache will be given / io->dedup_table will be NULL
 *   pynqs_reduce_onepass          : the launch (memsets of the de-duplication table and counters included)
 *   pynqs_reduce_contract         : eloc[x] = sum_records w A(x') / A(x) (divide = 1) or sum_records w A(x') (divide = 0) and
 *                                   psi_x[x] = A(x), from the records (io->rec_w / srec_w: any weights in the records' slot
 *                                   layout) and the values A of the distinct list (psi_unique) and of the table (psi_table);
 *                                   one wave per walker, fixed order of additions.
 * Record link: >= 2^30 : row (link - 2^30) of the distinct list (the row was known when the record was written: the record's own new
 * determinant, or one whose winner had already published its row); 0 .. 2^30 - 1 : slot of the de-duplication table (its row number is
 * stored in the slot: the contraction looks it up); <= -2 : position -(link + 2) of the wave-function table; -1 : no amplitude
 * (capacity overflow).  Which of the first two forms a record gets depends on the launch's timing; both lead to the same row. */
typedef struct pynqs_reduce_io {
  int64_t cap_doubles;  /* in: compacted slots per segment after the fixed ones */
  int64_t cap_unique;   /* in: rows of uniq_onv / uniq_pm1 */
  int64_t dedup_slots;  /* in: power of two >= 2 * cap_unique, <= 2^30 */
  int32_t *rec_col;     /* [segments][fixed + cap_doubles] column of the record, -1 = empty slot */
  void *rec_w;          /* T, same shape: <x|H|x'> */
  uint64_t *rec_onv;    /* same shape x len (may be NULL) */
  int32_t *rec_link;    /* same shape */
  int32_t *seg_count;   /* [segments] kept doubles of the segment (may exceed cap_doubles: overflow) */
  int32_t *srec_col;    /* [nbatch][eps_sample]: drawn records (eps_sample > 0), -1 = unused slot */
  void *srec_w;         /* T: (c / N) sign(H) S */
  uint64_t *srec_onv;   /* may be NULL */
  int32_t *srec_link;
  double *row_sum;      /* [nbatch] S (may be NULL) */
  void *dedup_table;    /* out[2] bytes from the geometry call; NULL = no de-duplication: every record that the wave-function table
                           does not answer gets a row of its own in uniq_onv (cap_unique >= the number of records; the distinct-list
                           counter counts records).  E_loc is the same; worth it when nearly all x' are distinct anyway and the table
                           would be gigabytes (random probes there cost 10x the enumeration).  LIST forms only: cap_doubles <=
                           pynqs_reduce_onepass_list_capacity */
  uint64_t *uniq_onv;   /* [cap_unique][len] distinct determinants, order of first insertion */
  void *uniq_pm1;       /* [cap_unique][sorb] +1/-1 rows, element type pm1_dtype (may be NULL) */
  int32_t pm1_dtype;    /* PYNQS_F32 / PYNQS_F64 */
  int32_t lut_is_hash;  /* reserved, must be 1 */
  const void *lut_table;  /* pynqs_hash_build table of the wave-function keys, or NULL */
  int64_t lut_nkeys;
  int32_t *counters;    /* [4] out: distinct determinants needed, overflow bits (1 doubles, 2 table, 4 distinct list),
                           largest seg_count of an overflowing segment, reserved */
  const uint64_t *seed_dev; /* optional: a seed in DEVICE memory, added to `seed` (a captured HIP graph replays the launch with
                               the same arguments: the caller bumps this word between replays) */
  void *row_cache;      /* optional, eps_sample > 0: T[nbatch][ncomb] scratch.  The enumeration stores every matrix element there and the
                           draws read the row back (L2) instead of visiting the drawn tiles a second time: worth it when the draws are
                           dense in the row (1000 draws over Fe2S2's 7876 columns hit every tile); leave NULL for long rows */
  int32_t *uniq_parent; /* optional, [cap_unique]: the walker whose record put the row on the distinct list -- the row is that walker or a
                           single / double excitation of it, which lets an amplitude with cheap updates start from the walker's
                           intermediate values (pynqs_rbm_forward_children) */
  void *tile_scratch;   /* optional, eps_sample > 0 without row_cache: pynqs_reduce_plan.tile_scratch_bytes bytes.  The per-tile sums of
                           the sub-eps |H| and the tiles' draw counts then live there instead of the LDS (12 bytes per tile: 57 KB per
                           workgroup at sorb 120, which leaves one workgroup per CU); for rows of more than ~65536 columns */
  int64_t tile_scratch_bytes;
  float *row_f32;       /* optional, eps_sample > 0: float[nbatch][stride] scratch, stride = ncomb rounded up to a multiple of 16, 64-byte aligned
                           (pynqs_reduce_plan.row_f32_elements).  With it -- and in the form PYNQS_REDUCE_ROWOUT: rows of up to
                           8192 columns, Fe2S2 -- the enumeration leaves the row's sub-eps matrix elements there as float32 (kept columns: 0) and
                           the same workgroup then locates the N draws in it: segments of 16 columns, their sums in float64, one lane per draw
                           (binary search over the segments, 64 bytes of the row read back), hit counts by the rank of a column's bit in a bitmap.
                           P(column j) = float32(|H_j|) / sum of those (relative 6e-8 of the reference's |H_j| / S); the weight of a drawn record
                           is the reference's (c / N) sign(H_j) S with S summed in float64.  The drawn records fill the first slots of
                           srec_* in ascending column order.  row_cache / tile_scratch are not used then. */
  int32_t form;         /* 0: the launch decides its form from the buffers given.  Otherwise the pynqs_reduce_form of the caller's plan: the
                           launch must arrive at exactly this form from the buffers it was handed, else it returns PYNQS_EINVAL ("plan and
                           buffers disagree") before anything is enqueued */
} pynqs_reduce_io;
/* The kernel families of the front end (DESIGN.md section 4.3 has the table: when each is taken, what it reads).  Whether the tile sums of
 * a semi-stochastic call live in io->tile_scratch instead of the LDS is a flag beside the form (pynqs_reduce_plan.tile_sums_global). */
typedef enum pynqs_reduce_form {
  PYNQS_REDUCE_LOOKBACK = 1,    /* "lookback":    kept columns compacted by decoupled look-back; needs the de-duplication table */
  PYNQS_REDUCE_LIST = 2,        /* "list":        a segment's records in an LDS list, no draws */
  PYNQS_REDUCE_LIST_CACHE = 3,  /* "list_cache":  LIST, the draws read the row back from io->row_cache */
  PYNQS_REDUCE_LIST_REDRAW = 4, /* "list_redraw": LIST, the drawn tiles are enumerated a second time */
  PYNQS_REDUCE_FLUSH = 5,       /* "flush":       the list is emptied whenever it is nearly full (with draws: drawn tiles enumerated again) */
  PYNQS_REDUCE_FLUSH_ROW32 = 6, /* "flush_row32": flushing, the draws read the drawn tiles back from io->row_f32 */
  PYNQS_REDUCE_ROWOUT = 7       /* "rowout":      LIST with the row's float32 copy in io->row_f32 and sorted draws (short rows) */
} pynqs_reduce_form;
const char *pynqs_reduce_form_name(int form); /* the short names above; "?" for anything else.  PYNQS_OP_VERBOSE prints them */
/* What the decision depends on.  The last five are the caller's permissions and limits (pynqs_amd/reduce_front.py keeps them as module
 * constants): which optional buffers it is willing to allocate and up to which size, and the row length (columns; < 0: that of
 * pynqs_reduce_onepass_long_row) from which the tile sums of a semi-stochastic call leave the LDS. */
typedef struct pynqs_reduce_plan_request {
  int64_t nbatch, sorb, nele, noA, noB, dtype /* of the integrals: PYNQS_F32 / PYNQS_F64 */, eps_sample, cap_doubles;
  int64_t with_table, dedup_slots; /* whether io->dedup_table will be given; slots of that table (for table_bytes; 0: not asked) */
  int64_t allow_row_f32, row_f32_max_bytes, allow_row_cache, row_cache_max_bytes, tile_scratch_min_row;
} pynqs_reduce_plan_request;
/* The answer: the form pynqs_reduce_onepass takes when it is handed exactly the optional buffers named here, and its launch parameters.
 * The buffers are offered in this order: io->row_f32 where the call would use it (row_f32_form 1: whatever its size; 2: within
 * row_f32_max_bytes), else io->row_cache where the draws are dense in the row (eps_sample * 64 >= columns) and it is within
 * row_cache_max_bytes, then io->tile_scratch on rows of more than tile_scratch_min_row columns unless the row cache or the sorted-draws
 * form makes it useless.  The form depends on the offer; an offered buffer is not always read by the final form. */
typedef struct pynqs_reduce_plan {
  int64_t form, tile_sums_global; /* pynqs_reduce_form; 1: tile sums and draw counts in io->tile_scratch */
  int64_t serves, long_row;       /* 0: the front end has no form for this system (LDS), use the multi-pass entry points -- a coarser test
                                     than the decision: float64 integrals, any cap_doubles; 1: more columns than pynqs_reduce_onepass_long_row() */
  int64_t segments, nchunks, chunk_len, max_tiles, fixed;
  int64_t list_slots, lds_bytes, table_bytes; /* P; dynamic LDS per workgroup; bytes of a de-duplication table of request.dedup_slots slots */
  int64_t row_f32_form; /* what io->row_f32 was wanted for: 1 sorted draws, 2 flushing form, 0 not (2 stays when row_f32_max_bytes forbids it) */
  int64_t row_f32_elements, row_cache_elements, tile_scratch_bytes; /* to allocate: floats / elements of the integral dtype / bytes; 0: none */
} pynqs_reduce_plan;
int pynqs_reduce_onepass_plan(const pynqs_reduce_plan_request *request, pynqs_reduce_plan *plan);
int64_t pynqs_reduce_onepass_long_row(void); /* columns */
int pynqs_reduce_onepass_list_capacity(int64_t nbatch, int sorb, int nele, int noA, int noB, int dtype, int eps_sample,
                                       int with_row_cache, int without_table, int64_t *cap_doubles);
int pynqs_reduce_onepass(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const void *plan,
                         int dtype, double eps, int eps_sample, uint64_t seed, const pynqs_reduce_io *io, void *stream);
/* the same with the tile loop of the short-row semi-stochastic kernel (PYNQS_REDUCE_ROWOUT) chosen per call; the
 * other forms of the front end have one tile loop and ignore the choice.  PYNQS_ROWOUT_TILEWISE (what pynqs_reduce_onepass takes): the tile
 * sums by cross-lane moves of a fixed pattern and formed behind the next tile's gathers, the kept columns of a full tile of doubles handed
 * to the list together (one LDS atomic per tile).  PYNQS_ROWOUT_PER_COLUMN: __shfl_xor butterflies in front of the next tile, one hand-off
 * per kept column.  Same additions in the same order, records
 * placed by bitmap rank: every output is the same bit for bit (the distinct list's order follows the launch's timing under either). */
#define PYNQS_ROWOUT_TILEWISE 0
#define PYNQS_ROWOUT_PER_COLUMN 1
int pynqs_reduce_onepass_form(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const void *plan,
                              int dtype, double eps, int eps_sample, uint64_t seed, const pynqs_reduce_io *io, int form, void *stream);
/* the wave sums and scans of the front end on caller-supplied data, one wave per 64 values, every lane's result (for tests):
 * what = 0: float64, the fixed-pattern butterfly; 1: float64, the __shfl_xor butterfly; 2 / 3: the same for uint32; 4: uint32 inclusive
 * scan by fixed-pattern moves.  in / out: device pointers to nwaves * 64 values of 8 (what 0, 1) or 4 bytes. */
int pynqs_debug_wave_sum(const void *in, void *out, int64_t nwaves, int what, void *stream);
int pynqs_reduce_contract(int64_t nbatch, int sorb, int nele, int noA, int noB, int dtype, int eps_sample,
                          const pynqs_reduce_io *io, const double *psi_unique, const double *psi_table, int psi_is_complex,
                          int divide, double *eloc, double *psi_x, void *stream);
/* the same with the kernel chosen per call: PYNQS_CONTRACT_BATCHED reads a slot's
 * column first, loads weight and link of live slots only and keeps the loads of several slots per lane in flight; PYNQS_CONTRACT_SERIAL
 * visits a lane's slots one at a time.  Same additions in the same order: eloc and psi_x are the same bit for bit. */
#define PYNQS_CONTRACT_BATCHED 0
#define PYNQS_CONTRACT_SERIAL 1
/* A flag beside the form, for either (form | PYNQS_CONTRACT_BY_XCD): which walkers a workgroup serves.  Without it workgroup b
 * of B serves walker group b (a group: the walkers of one workgroup, consecutive).  With it, it serves group
 * pynqs_reduce_contract_group(b, B): the workgroups b = j (mod 8) -- which the hardware has been seen to deal to one XCD, and with it one
 * L2 -- share a contiguous range of groups, whose rows of psi_unique are neighbours.  Only speed may depend on that dealing: the map is a
 * permutation of 0 .. B-1 for every B, and eloc and psi_x do not change by a bit. */
#define PYNQS_CONTRACT_BY_XCD 0x100
/* (pynqs_reduce_contract takes PYNQS_CONTRACT_BATCHED | PYNQS_CONTRACT_BY_XCD: profiles/contract_stream_ab.txt) */
/* g = j (B >> 3) + min(j, B & 7) + (b >> 3) with j = b & 7, for 0 <= b < B (-1 outside); host code, no device needed */
int64_t pynqs_reduce_contract_group(int64_t b, int64_t B);
int pynqs_reduce_contract_form(int64_t nbatch, int sorb, int nele, int noA, int noB, int dtype, int eps_sample,
                               const pynqs_reduce_io *io, const double *psi_unique, const double *psi_table, int psi_is_complex,
                               int divide, double *eloc, double *psi_x, int form, void *stream);
/* ---- the draw law of the short-row form (pynqs_reduce_onepass in its form PYNQS_REDUCE_ROWOUT:
 * rows of at most 8192 columns, at most 16383 draws, the kept records within the list; pynqs_amd/csrc/reduce_draw.h).  This form's random
 * STREAM is part of the contract: which columns walker i draws, and how often, is a pure function of (seed, *io->seed_dev, i, the row).
 * tests/reduce_replay.py replays it on the host; tests/test_gpu_reduce_replay.py compares every record.
 *  - Hash: mix64 = the splitmix64 finaliser (pynqs_amd/csrc/mix64.h), all arithmetic modulo 2^64.
 *  - Key of walker i (its index in the call, from 0):  key = mix64((seed + seed_dev) ^ mix64(i)),  seed_dev = *io->seed_dev as the launch
 *    reads it from device memory (0 when io->seed_dev is NULL).  A caller that replays the launch from a HIP graph bumps that word between
 *    replays (reduce_front.ReduceStep: +1 per replay, inside the graph), so that replay m draws with seed + seed_dev_m.
 *  - Draw k = 0 .. N - 1 (N = eps_sample) of the walker:  r_k = mix64(key ^ ((k + 1) * 0x9e3779b97f4a7c15)),  u_k = (r_k >> 11) * 2^-53 in
 *    [0, 1): a 53-bit uniform, exact in double.
 *  - Widths, in the reference's column order (column 0 the diagonal, then get_comb_tensor's singles and doubles): w32_j = float32(|H_j|),
 *    round to nearest, for the sub-eps columns -- |H_j| < eps compared in the integral dtype; with eps <= 0 nothing is kept and every
 *    column is sub-eps -- and 0 for the kept ones.  With float32 integrals the widths are the elements' magnitudes themselves.
 *    C_j = w32_0 + ... + w32_j,  S' = C_last.  A float64 element below the float32 range has width 0 and is never drawn.
 *  - Boundary rule: draw k chooses the column j with  C_{j-1} <= u_k S' < C_j  (C_{-1} = 0): the first column whose running sum exceeds
 *    the target.  A column of width zero (kept, or an exact zero) is never chosen.  P(column j) = w32_j / S', which is the reference's
 *    |H_j| / S (torch.multinomial(prob, N, replacement=True), vmc/energy/eloc.py:263-296) to 6e-8 relative.
 *  - Rounding: the kernel forms S', the starting sum of a segment of 16 columns and the running sum inside the segment in float64, each a
 *    sum of at most ncomb non-negative terms in a fixed order, so its choice is the rule's whenever the target is farther than
 *    2^-51 (ncomb + 64) S' from both ends of the column's interval; nearer than that it may be the neighbouring column of positive width,
 *    nothing else.  Fallbacks when rounding takes the target past the last positive width of its segment: that last column; when the
 *    segment has no width at all: the nearest column of positive width after it, else before it.  A row without any width (S' = 0) draws
 *    nothing and leaves all N slots at -1; its kept records and row_sum = 0 are written as usual.
 *  - Records: one per distinct drawn column, in the first slots of the walker's N, ascending columns (the reference's
 *    unique(sorted=True)); a column drawn c times carries  (c / N) sign(H_j) S  in the integral dtype,  S = io->row_sum = the float64 sum of
 *    the exact sub-eps |H_j| (within ncomb 2^-52 relative of the exact sum; the weight within (ncomb + 2) 2^-52 relative).
 *  - Limits: ncomb <= 8192 columns and N <= 16383 draws (a record waits as count << 16 | sign << 15 | column); beyond either the call
 *    takes one of the forms below.
 * The other semi-stochastic forms -- the flushing and look-back forms of this entry point, the LIST form with
 * io->row_cache or io->tile_scratch, and the multi-pass pynqs_reduce_count_sums / pynqs_reduce_sample -- draw HIERARCHICALLY: first the tile
 * (in proportion to the tiles' sums of sub-eps |H|), then the column inside the tile in the tile's enumeration order, with streams keyed by (seed, walker
 * or slot, tile, k).  Only their LAW is contractual -- P(column j) = |H_j| / S, N draws per walker with replacement, the same records and
 * weights --, not their stream: it may change with the tiling. */

/* ---- the RBM amplitudes themselves on a LIST of determinants (kernels_rbm_forward.hip): psi(x) of vmc/ansatz/rbm/rbm.py:186-211 from the
 * packed bits, one lane per determinant, nothing but the result written.  The amplitude forward of the REDUCE local energy (`Func` on the
 * distinct x', vmc/energy/flip.py:44-50) when the ansatz is an RBM: the PyTorch module's GEMM + element-wise kernels on [n, nhidden] arrays
 * cost 3.5 ms per 1.5 M determinants, this kernel 0.3-0.5 ms.
 *   flavour PYNQS_RBM_REAL / _TANH: weights double[nhidden][sorb], hidden_bias double[nhidden], visible_bias double[sorb] or NULL; psi double[n]
 *   flavour PYNQS_RBM_PHASE       : same parameters; psi double[n][2] = exp(i (a.x + sum_h ln 2cosh theta_h))
 *   flavour PYNQS_RBM_COMPLEX     : weights double[nhidden][sorb][2], hidden_bias double[nhidden][2], visible_bias double[sorb][2] or NULL
 *                                   (the reference's params_* layout, rbm_type "complex"); psi double[n][2] */
#define PYNQS_RBM_COMPLEX 4
int pynqs_rbm_forward(const uint64_t *onv, int64_t n, int sorb, const double *weights, const double *hidden_bias,
                      const double *visible_bias, int nhidden, int flavour, double *psi, void *stream);

/* ---- the energy-gradient estimator for RBM amplitudes, analytically (kernels_rbm_grad.hip; vmc/grad/energy_grad.py:118-184, "AD" method:
 *   loss = 2 Re sum_n p_n conj(ln psi(x_n)) (E_loc(x_n) - <E> c_n); the reference calls loss.backward() on it).
 * For psi = exp(a.x) prod_h 2cosh(theta_h), theta = b + W x (vmc/ansatz/rbm/rbm.py:186-211):
 *   d loss / d theta_k = 2 Re G_k (real parameters) or (2 Re G_k, -2 Im G_k) for a complex parameter stored as (re, im),
 *   G_k = sum_n conj(f_n) O_k(x_n),  f_n = p_n (E_loc(x_n) - <E> c_n),  O = (x_o, tanh theta_h, tanh theta_h x_o).
 *   flavour: PYNQS_RBM_REAL (parameters double[nhidden][sorb], [nhidden], [sorb]) or PYNQS_RBM_COMPLEX (the same with a trailing [2]);
 *   prob double[n]; eloc double[n] or (eloc_is_complex) double[n][2]; e_total: DEVICE pointer to <E> (1 or 2 doubles, as eloc);
 *   pow: c_n double[n] (extra_psi_pow) or NULL for 1; visible_bias / grad_visible_bias may be NULL.
 *   grad_*: same shapes as the parameters (overwritten); loss (may be NULL): the loss above, ln psi on torch.log's principal branch.
 *   workspace: pynqs_rbm_grad_workspace(n, sorb, nhidden, flavour) bytes.  Sums run in a fixed order: bit-reproducible.               */
/* ---- RBM amplitudes of the DISTINCT x' of a REDUCE front end, from their parents (kernels_rbm_forward.hip): row r of the distinct list is
 * walker parent[r] with at most four orbitals flipped, and  prod_h 2cosh(theta_h) = exp(sum_h theta_h) prod_h (1 + q_h),  q_h = exp(-2 theta_h):
 * flipping orbital o to x'_o = +-1 multiplies q_h by the table entry exp(-+4 W_ho).  A child costs 4 table multiplications per hidden unit:
 * no exponential, no sine, no loop over the orbitals (Fe2S2, 1.5 M rows x 40 complex hidden units: 0.60 ms from scratch).
 *   pynqs_rbm_children_table_bytes : [host] size of the table for nwalkers parents (-1 on bad arguments)
 *   pynqs_rbm_children_prepare     : table <- the parents' q_h, sum_h theta_h, a.x and the parameters' factor table
 *   pynqs_rbm_forward_children     : psi[r] for r < min(*count_dev, n) (count_dev may be NULL: all n rows; rows past the count are left alone)
 *   pynqs_rbm_forward_children_supported : 1 for every valid (sorb, nhidden, flavour), else 0.  A factor table ((2 sorb + 1) x
 *                                    ((nhidden + 2) | 1) entries of 8 bytes, 16 for complex parameters) of at most 64 KB is kept in LDS, a
 *                                    thread per row; a larger one (sorb x nhidden above ~64 x 64) is read from the L2 by one wave per
 *                                    row, the lanes over the hidden units
 *   pynqs_rbm_forward_children_geometry : [host] the launch of pynqs_rbm_forward_children for n rows: out[0] = form (0: table in LDS,
 *                                    1: a wave per row), out[1] = workgroups launched (capped: they stride over the rows), out[2] = rows
 *                                    the grid covers per sweep on the table route, out[3] = rows per sweep on the from-scratch route (the
 *                                    flag raised: a thread per row in both forms).  The expressions the launch itself uses.
 * Flavours and parameter layouts as pynqs_rbm_forward.  exp(-2 theta_h) is formed for the parents: if some Re theta_h < -340 the prepare
 * step raises a flag in the table and pynqs_rbm_forward_children computes every row from scratch instead (pynqs_rbm_forward's
 * algorithm inside the same kernel).  Below that, negative theta_h still make the factors 1 + q_h large (e^100 at theta_h = -50): a row
 * whose product of them, or whose q_h after the flips, leaves the range of a double is detected (the product is inf or nan) and computed
 * from scratch inside the same launch, as is a row that flips an orbital with |4 Re W_ho| > 80 (its table entry is stored as nan); the
 * other rows keep the parents' route.  Such rows cost a from-scratch evaluation on top: a model with many hidden units at theta_h << -40
 * is served no faster than by pynqs_rbm_forward.  For every row whose psi is a finite double the value obeys the rounding bound of
 * pynqs_rbm_forward, |psi / psi_exact - 1| <= 2^-53 (sorb + nhidden + 16) cond(x), cond(x) = 1 + sum_h |tanh theta_h| (|b_h| + sum_o
 * |W_ho|) + sum_o |a_o| (tests/rbm_exact.py; typically 1e-14 relative, a factor 2cosh(theta_h) near zero amplifies it through cond).      */
int64_t pynqs_rbm_children_table_bytes(int64_t nwalkers, int sorb, int nhidden, int flavour);
int pynqs_rbm_children_prepare(const uint64_t *walkers, int64_t nwalkers, int sorb, const double *weights, const double *hidden_bias,
                               const double *visible_bias, int nhidden, int flavour, void *table, void *stream);
int pynqs_rbm_forward_children(const uint64_t *onv, int64_t n, const int32_t *count_dev, const int32_t *parent,
                               const uint64_t *walkers, int64_t nwalkers, const void *table, int sorb, const double *weights,
                               const double *hidden_bias, const double *visible_bias, int nhidden, int flavour, double *psi,
                               void *stream);
int pynqs_rbm_forward_children_supported(int sorb, int nhidden, int flavour);
int pynqs_rbm_forward_children_geometry(int64_t n, int sorb, int nhidden, int flavour, int64_t *out4);
/* the same with the schedule of the LDS kernel chosen per call (pynqs_rbm_forward_children and ..._stamped take PYNQS_CHILDREN_CHUNKED):
 *   PYNQS_CHILDREN_CHUNKED : eight hidden units at a time -- the parent's q_h of a chunk loaded together, the factors read a slot at a
 *                            time for the chunk, the eight q_h chains side by side; the nhidden % 8 units left over one by one.  REAL,
 *                            TANH and PHASE also request the next chunk's q_h before this chunk's arithmetic; PYNQS_RBM_COMPLEX does not
 *                            (a second buffer of q_h does not fit its registers: it spilled and ran slower);
 *   PYNQS_CHILDREN_PER_UNIT: one hidden unit after the other, each waiting for its own loads.
 * The same operations on the same operands in the same order (q_h times its four factors in slot order, the product *= 1 + q_h in ascending
 * h, renormalised after every eight): psi is the same bit for bit.  The wave form (a table beyond the LDS) has one schedule and ignores
 * `form`; any other value is PYNQS_EINVAL.
 * In the LDS form (both schedules) a row that has to be computed from scratch is marked in `psi` by a first loop and computed by a second:
 * `psi` serves as scratch for the length of the launch and must not be read concurrently; rows at and past the count stay untouched. */
#define PYNQS_CHILDREN_CHUNKED 0
#define PYNQS_CHILDREN_PER_UNIT 1
int pynqs_rbm_forward_children_form(const uint64_t *onv, int64_t n, const int32_t *count_dev, const int32_t *parent,
                                    const uint64_t *walkers, int64_t nwalkers, const void *table, int sorb, const double *weights,
                                    const double *hidden_bias, const double *visible_bias, int nhidden, int flavour, int form, double *psi,
                                    void *stream);
/* The same pair with ONE launch for the prepare step (the same table bit for bit).  Within one launch the flag cannot be reset and then
 * raised, so a parent out of range stores the call's `stamp` there and pynqs_rbm_forward_children_stamped takes the flag for raised only if
 * it holds its own stamp: pass the same number in [1, 2^53) to both calls and a different one to every prepare call that may meet the same
 * table memory (a process-wide call counter).  A stale stamp or the garbage of a fresh buffer reads as "not raised"; garbage that equals
 * the stamp sends the call down the from-scratch path, which is right for every input.  Do not mix the stamped and the plain entry points
 * on one table. */
int pynqs_rbm_children_prepare_stamped(const uint64_t *walkers, int64_t nwalkers, int sorb, const double *weights,
                                       const double *hidden_bias, const double *visible_bias, int nhidden, int flavour, uint64_t stamp,
                                       void *table, void *stream);
int pynqs_rbm_forward_children_stamped(const uint64_t *onv, int64_t n, const int32_t *count_dev, const int32_t *parent,
                                       const uint64_t *walkers, int64_t nwalkers, const void *table, int sorb, const double *weights,
                                       const double *hidden_bias, const double *visible_bias, int nhidden, int flavour, uint64_t stamp,
                                       double *psi, void *stream);
int pynqs_rbm_forward_children_stamped_form(const uint64_t *onv, int64_t n, const int32_t *count_dev, const int32_t *parent,
                                            const uint64_t *walkers, int64_t nwalkers, const void *table, int sorb, const double *weights,
                                            const double *hidden_bias, const double *visible_bias, int nhidden, int flavour, uint64_t stamp,
                                            int form, double *psi, void *stream);

int64_t pynqs_rbm_grad_workspace(int64_t n, int sorb, int nhidden, int flavour);
int pynqs_rbm_grad(const uint64_t *onv, int64_t n, int sorb, const double *weights, const double *hidden_bias,
                   const double *visible_bias, int nhidden, int flavour, const double *prob, const double *eloc,
                   int eloc_is_complex, const double *e_total, const double *pow, double *grad_weights,
                   double *grad_hidden_bias, double *grad_visible_bias, double *loss, void *workspace, void *stream);
/* the same; loss_copy (may be NULL) receives the loss a second time, e.g. a fresh one-element tensor for the caller to return while
 * `loss` stays inside its flat all-reduce buffer: no copy launch */
int pynqs_rbm_grad_loss(const uint64_t *onv, int64_t n, int sorb, const double *weights, const double *hidden_bias,
                        const double *visible_bias, int nhidden, int flavour, const double *prob, const double *eloc,
                        int eloc_is_complex, const double *e_total, const double *pow, double *grad_weights,
                        double *grad_hidden_bias, double *grad_visible_bias, double *loss, double *loss_copy, void *workspace,
                        void *stream);
/* the same with the schedule of the first kernel chosen per call (the two entry points above take PYNQS_GRAD_ONEPASS and block 0):
 *   PYNQS_GRAD_ONEPASS: the theta chains of 64 hidden units at a time run side by side, W of those units staged in LDS where it fits;
 *   PYNQS_GRAD_TWOPASS: passes of 32 hidden units, W from global memory.  Gradient and loss are the same bit for bit.
 *   block: threads per workgroup, 256 or 512; 0: 512 unless the environment says PYNQS_RBM_GRAD_BLOCK=256. */
#define PYNQS_GRAD_ONEPASS 0
#define PYNQS_GRAD_TWOPASS 1
int pynqs_rbm_grad_loss_form(const uint64_t *onv, int64_t n, int sorb, const double *weights, const double *hidden_bias,
                             const double *visible_bias, int nhidden, int flavour, const double *prob, const double *eloc,
                             int eloc_is_complex, const double *e_total, const double *pow, double *grad_weights,
                             double *grad_hidden_bias, double *grad_visible_bias, double *loss, double *loss_copy, void *workspace,
                             int schedule, int block, void *stream);

/* ---- stochastic reconfiguration for RBM amplitudes, matrix-free (kernels_rbm_sr.hip; vmc/grad/sr.py with vmc/grad/_jacobian.py, the
 * reference's `sr=True`, which builds a dense P x P matrix and inverts it) ---------------------------------------------------------------
 * Modules and parameter layouts as pynqs_rbm_grad: PYNQS_RBM_REAL (weights double[nhidden][sorb], hidden_bias [nhidden], visible_bias
 * [sorb]) or PYNQS_RBM_COMPLEX (the same with a trailing [2] = (re, im)).
 *  - Real parameter vector: the stored numbers in the order weights, hidden_bias, visible_bias, P_real = P or 2 P doubles with
 *    P = nhidden sorb + nhidden + sorb.  Every vector below (obar, v, y, rhs, d, r, p) is ONE flat buffer of this layout.
 *  - O_nk = d ln psi(x_n) / d theta_k = (tanh theta_h x_o, tanh theta_h, x_o), theta = b + W x (no dependence on the visible bias); the two
 *    real derivatives of a complex parameter stored as (re, im) are (O_nk, i O_nk).
 *  - Obar_k = sum_n p_n O_nk, p = prob (real; sums to 1 over all ranks; per rank pre-scaled by the world size, so every cross-rank sum is
 *    an all-reduce SUM divided by the world size).  obar holds (Re, Im) for pairs.
 *  - S = Re(<O* O> - <O*><O>) on the real parameters: the reference's S_kk (sr.py:87-117) for real parameters; for (re, im) pairs the
 *    real form [[A, -B], [B, A]] of the Hermitian matrix <O* O>_c = A + i B of the holomorphic parameters (the reference's
 *    inv(S).real @ F.real is not defined for its own complex layout, its "TODO: S-1 is complex or real").  S is symmetric, >= 0.
 *  - Product, z_k = v_k or v_k,re + i v_k,im:
 *      c_n = sum_k (O_nk - Obar_k) z_k = x_n . z_a + sum_h tanh theta_nh (z_b,h + sum_o z_W,ho x_no) - Obar . z,
 *      y_k = sum_n p_n conj(O_nk) c_n,      (S v)_k = y_k  or  (Re y_k, Im y_k).
 *  - The SR direction d solves (S + diag_shift I) d = F, F = the gradient exactly as pynqs_rbm_grad returns it (2 Re G, -2 Im G), the
 *    reference's F_i = 2 Re(<E_loc O_i*> - <E_loc><O_i*>); diag_shift 0.02 is the reference's default.
 *   pynqs_rbm_sr_workspace : [host] bytes of the workspace for n walkers (-1 on bad arguments): the tanh table, double[nhidden][n] (x2:
 *        (re, im)), walkers fastest; then the workgroups' partial sums (ceil(n / 32) x P_real doubles, the largest temporary besides the
 *        table); then Obar . z.  Nothing of size n x P or P x P.
 *   pynqs_rbm_sr_prepare   : once per solve: tanh theta -> the table (e = exp(-2 |Re theta|): no overflow), obar <- THIS rank's
 *        sum_n p_n O_nk.  n = 0 gives obar = 0.
 *   pynqs_rbm_sr_matvec    : y <- THIS rank's y as defined above for the vector v, from the packed bits and the table; obar: the
 *        ALL-REDUCED Obar, so Obar . z needs no communication.  v and y must not overlap.  n = 0 gives y = 0.
 *   pynqs_rbm_sr_cg_step   : the vector part of conjugate gradients on (S + diag_shift) d = rhs, np = P_real, one workgroup, scalars
 *        double[PYNQS_SR_NSCALARS] in device memory (no host synchronisation):
 *          PYNQS_SR_CG_INIT      d = 0, r = p = rhs, rho = |rhs|^2, iterations = 0; done and converged at once when rhs = 0
 *          PYNQS_SR_CG_STEP      after y <- matvec(p) (all-reduced SUM over the ranks): Ap = y inv_world + diag_shift p (left in y),
 *                                alpha = rho / p.Ap, d += alpha p, r -= alpha Ap, rho' = r.r, p = r + (rho' / rho) p, iterations += 1;
 *                                done when rho' <= tol^2 |rhs|^2 (or p.Ap <= 0: breakdown).  A no-op once done is set, so that the
 *                                host may enqueue several iterations between read-backs of the scalars.
 *          PYNQS_SR_CG_RESIDUAL  after y <- matvec(d): r = rhs - (y inv_world + diag_shift d), the TRUE residual, |r|^2 -> PYNQS_SR_TRUE2;
 *                                converged and done when |r|^2 <= tol^2 |rhs|^2, else p = r, rho = |r|^2 and done is cleared: the
 *                                iteration goes on from d (the recurrence's residual drifts by rounding over hundreds of steps).
 * Every sum runs in a fixed order (two stages over the walkers, a tree over the parameters): all results are bit-reproducible.        */
#define PYNQS_SR_RHO 0       /* r.r of the recurrence */
#define PYNQS_SR_RHS2 1      /* |rhs|^2 */
#define PYNQS_SR_DONE 2      /* 0.0 / 1.0 */
#define PYNQS_SR_ITER 3      /* iterations performed (a whole number) */
#define PYNQS_SR_TRUE2 4     /* the last true |r|^2 (PYNQS_SR_CG_RESIDUAL) */
#define PYNQS_SR_PAP 5       /* the last p.Ap */
#define PYNQS_SR_CONVERGED 6 /* 0.0 / 1.0: the TRUE residual met the tolerance */
#define PYNQS_SR_BREAKDOWN 7 /* 1.0: p.Ap <= 0 or not a number */
#define PYNQS_SR_NSCALARS 8
#define PYNQS_SR_CG_INIT 0
#define PYNQS_SR_CG_STEP 1
#define PYNQS_SR_CG_RESIDUAL 2
int64_t pynqs_rbm_sr_workspace(int64_t n, int sorb, int nhidden, int flavour);
int pynqs_rbm_sr_prepare(const uint64_t *onv, int64_t n, int sorb, const double *weights, const double *hidden_bias, int nhidden,
                         int flavour, const double *prob, void *workspace, double *obar, void *stream);
int pynqs_rbm_sr_matvec(const uint64_t *onv, int64_t n, int sorb, int nhidden, int flavour, const double *prob, const void *workspace,
                        const double *obar, const double *v, double *y, void *stream);
int pynqs_rbm_sr_cg_step(int mode, int64_t np, double *y, const double *rhs, double *d, double *r, double *p, double *scalars,
                         double inv_world, double diag_shift, double tol, void *stream);
/* The same for the Jastrow-RBM, psi(x) = exp(a.x + x^T M x) prod_h 2cosh(theta_h) (pynqs_jrbm_forward; all parameters real).  The parameter
 * vector gains the jastrow block: weights [nhidden][sorb], hidden_bias, visible_bias, jastrow [sorb][sorb]; P = nhidden sorb + nhidden +
 * sorb + sorb^2, and obar, v, y (and the vectors of pynqs_rbm_sr_cg_step, which serves this solve unchanged with np = P) are flat
 * double[P] of this layout.  O_n = (tanh theta_nh x_no, tanh theta_nh, x_no, x_ni x_nj); with Z the jastrow block of v,
 *      c_n = x_n . z_a + sum_h tanh theta_nh (z_b,h + sum_o z_W,ho x_no) + x_n^T Z x_n - Obar . z,      y_k = sum_n p_n O_nk c_n;
 * the first three blocks of y are those of pynqs_rbm_sr_matvec with this c_n, and y_M[i][j] = sum_n p_n c_n x_ni x_nj.
 *  - S does not depend on M.  It is singular on the jastrow block by construction: O_ii = 1 (row and column ii of S are zero, so
 *    d_ii = F_ii / diag_shift), O_ij = O_ji, and with fixed particle numbers sum_j x_i x_j is proportional to x_i; diag_shift
 *    regularises all of it and conjugate gradients from zero stay in the range of S.
 *  - Only the symmetric part of Z reaches c_n: the kernel evaluates x^T Z x = sum_i Z_ii + sum_{i<j} (Z_ij + Z_ji) x_i x_j.
 *  - The jastrow block of y (and of obar) is bit-symmetric, y_M[i][j] == y_M[j][i]: one sum is formed for i <= j and written twice.
 *   pynqs_jrbm_sr_workspace : [host] bytes (-1 on bad arguments): the tanh table double[nhidden][n], the workgroups' partial sums
 *        (ceil(n / 32) x (nhidden (sorb + 1) + sorb + ceil(sorb / 2) (sorb + 1)) doubles: the jastrow block as its triangle), Obar . z.
 *   pynqs_jrbm_sr_prepare   : as pynqs_rbm_sr_prepare (the table does not depend on M); obar gains sum_n p_n x_ni x_nj.  n = 0: obar = 0.
 *   pynqs_jrbm_sr_matvec    : as pynqs_rbm_sr_matvec.  Z is staged in LDS (symmetrised) for sorb <= 128 and read from global memory
 *        above.  v and y must not overlap.  n = 0: y = 0.                                                                            */
int64_t pynqs_jrbm_sr_workspace(int64_t n, int sorb, int nhidden);
int pynqs_jrbm_sr_prepare(const uint64_t *onv, int64_t n, int sorb, const double *weights, const double *hidden_bias, int nhidden,
                          const double *prob, void *workspace, double *obar, void *stream);
int pynqs_jrbm_sr_matvec(const uint64_t *onv, int64_t n, int sorb, int nhidden, const double *prob, const void *workspace,
                         const double *obar, const double *v, double *y, void *stream);

/* ---- many-chain Metropolis sampling (vmc/sample.py:480-569, Sampler.MCMC; the reference runs one chain in a Python loop) -------------
 * Semantics shared by both entry points (and by pynqs_amd/mcmc.py, which drives them):
 *  - nchains independent chains; chain i of a call has the global index c = chain_base + i (c < 2^32).  Steps are numbered t = 0, 1, ...
 *    from the sampler's start, so successive calls continue the random streams.
 *  - Proposal of step t, chain c: pynqs_spin_flip_rand's draw with offset = (t << 32) + chain_base and the chain as the launch index,
 *      r0 = umulhi(mix64(mix64(seed) ^ mix64((t << 32) + c)), nsd + 1),   mix64 = the splitmix64 finaliser (pynqs_amd/csrc/mix64.h);
 *    r0 == 0 keeps the state, any other r0 applies excitation rank r0 - 1 (a uniform single or double excitation, or no move).
 *  - No Hastings factor: the proposal is symmetric.  nsd depends only on (sorb, noA, noB), and rank -> excitation is a bijection onto
 *    the singles and doubles of any determinant with noA alpha and noB beta electrons (the reference's same-spin `idx % noAA` quirk is a
 *    cyclic shift of the hole-pair index inside each virtual pair, still a bijection), so x -> x' and x' -> x have the same probability.
 *  - Acceptance draw: u = ((h >> 11) + 0.5) * 2^-53 in (0, 1] (double arithmetic, in this order),
 *      h = mix64(mix64(seed ^ PYNQS_MCMC_ACCEPT_KEY) ^ mix64((t << 32) + c)).
 *    The proposal is accepted iff u <= |psi(x')|^2 / |psi(x)|^2 (the reference's random() <= min(1, ratio)); if |psi(x)| == 0 every
 *    proposal is accepted (the reference's ratio is inf or nan there, and min(1.0, .) accepts).  The ratio is that of the amplitudes
 *    for every finite nonzero |psi(x)|, however small or large (not of their squares in double, which under- or overflow).
 *    Non-finite amplitudes (a part inf or nan; only pynqs_mcmc_accept can be given one): a proposal with one is rejected, also from a
 *    state of amplitude zero, and a state with one accepts every proposal of finite amplitude, as a state of amplitude zero does.  (The
 *    reference's min(1.0, nan) accepts, its finite / inf = 0 rejects: a chain would enter such states and could stick there.)
 *  - Recording (pynqs_amd/mcmc.py): the first n_therm steps are discarded, then n_sample steps run and the state after every
 *    `every`-th of them is recorded; accepted moves are counted over those n_sample steps only.  With nchains = 1 and every = 1 this is
 *    Sampler.MCMC step for step, except for the random numbers (the reference's mt19937 / XORWOW statics cannot be reproduced anyway).
 *
 *   pynqs_mcmc_rbm : `nsteps` steps t = t0 .. t0 + nsteps - 1 of every chain in ONE launch, psi an RBM amplitude (flavours of
 *        pynqs_rbm_forward): states uint64[nchains][len], read and written in place.  table: the RBM table (pynqs_rbm_table_build) for
 *        PYNQS_RBM_REAL / TANH / PHASE, the complex table (pynqs_crbm_table_build) for PYNQS_RBM_COMPLEX.  records (may be NULL):
 *        uint64[nsteps / every][nchains][len], row r = the states after step t0 + (r + 1) every - 1 (chain fastest).  n_accept (may be
 *        NULL): int64[nchains], += the moves accepted in this launch.  lnpsi (may be NULL): double[nchains] <- ln|psi| of the final
 *        states (pRBM: 0; every pRBM proposal is accepted, |psi| = 1).  Each chain's hidden-unit state is recomputed from the parameters
 *        at the start of the launch; keep launches short (the Python layer bounds the steps per launch).
 *   pynqs_mcmc_rbm_supported : 1 if (sorb, nhidden, flavour) has a fused kernel (nhidden <= 512, a valid table layout), else 0.
 *   pynqs_mcmc_jrbm : pynqs_mcmc_rbm for the real RBM times a two-body Jastrow factor, psi(x) = exp(a.x + x^T M x) prod_h 2cosh(theta_h)
 *        (pynqs_eloc_jrbm's amplitude).  rbm_table: pynqs_rbm_table_build; jastrow_table: pynqs_jastrow_table_build, of which the block
 *        S = M + M^T (zero diagonal) and tr M are read.  Every other argument, the random streams, records, n_accept and lnpsi as for
 *        pynqs_mcmc_rbm with PYNQS_RBM_REAL.  With F the 2 or 4 flipped orbitals and x the state before the move,
 *            ln|psi_J(x')| - ln|psi_J(x)| = -2 sum_{i in F} x_i r_i + 4 sum_{i<j in F} S_ij x_i x_j,    r_i = sum_j S_ij x_j,
 *        r_i summed anew at every step (at most 4 ceil(sorb / G) loads and fma per lane, G = the lanes of a chain), nothing of the
 *        Jastrow factor kept between steps; at the start of a launch ln|psi| takes tr M + sum_{i<j} S_ij x_i x_j.  With M = 0 the
 *        decisions and lnpsi are pynqs_mcmc_rbm's bit for bit.
 *   pynqs_mcmc_jrbm_supported : 1 where pynqs_mcmc_rbm_supported with PYNQS_RBM_REAL holds and sorb has a Jastrow table, else 0.
 *   pynqs_mcmc_jrbm_form : host only, the shape alone decides: bit 0 = the RBM table is copied to LDS (it is at most 64 KiB, as in
 *        pynqs_mcmc_rbm), bit 1 = S (sorb^2 doubles) too (both together within the 64 KiB); so 3, 1 or 0, and -1 where unsupported.
 *   pynqs_mcmc_accept : step t of any ansatz, after pynqs_spin_flip_rand(states, ..., seed, (t << 32) + chain_base, proposals).
 *        psi / psi_proposals: double[nchains] or, with is_complex, (re, im) pairs; states and psi take the proposals' values where the
 *        move is accepted; n_accept (may be NULL) is bumped there; record_row (may be NULL): uint64[nchains][len] <- the states after
 *        the step.                                                                                                                      */
#define PYNQS_MCMC_ACCEPT_KEY 0x243F6A8885A308D3ull
int pynqs_mcmc_rbm_supported(int sorb, int nhidden, int flavour);
int pynqs_mcmc_rbm(uint64_t *states, int64_t nchains, int sorb, int noA, int noB, const void *table, int nhidden, int flavour,
                   uint64_t seed, uint64_t chain_base, uint64_t t0, int nsteps, int every, uint64_t *records, int64_t *n_accept,
                   double *lnpsi, void *stream);
int pynqs_mcmc_jrbm_supported(int sorb, int nhidden);
int pynqs_mcmc_jrbm_form(int sorb, int nhidden);
int pynqs_mcmc_jrbm(uint64_t *states, int64_t nchains, int sorb, int noA, int noB, const void *rbm_table, const void *jastrow_table,
                    int nhidden, uint64_t seed, uint64_t chain_base, uint64_t t0, int nsteps, int every, uint64_t *records,
                    int64_t *n_accept, double *lnpsi, void *stream);
int pynqs_mcmc_accept(uint64_t *states, double *psi, const uint64_t *proposals, const double *psi_proposals, int64_t nchains,
                      int sorb, int is_complex, uint64_t seed, uint64_t chain_base, uint64_t t, uint64_t *record_row,
                      int64_t *n_accept, void *stream);

/* ---- reduced density matrices ---------------------------------------------------------------------------------------------------------
 * With E = sum_x w_x sum_k H[x,k] r_{x,k}, r = psi(x'_k) / psi(x), and H[x,k] linear in the packed integrals exactly as the local-energy
 * kernels read them:   rdm1[q sorb + p] = dE / dh1e[q sorb + p]  (h1e's layout, sorb^2 doubles),
 *                      rdm2[t]          = dE / dh2e[t]           (h2e's packed layout, pair (pair + 1) / 2 doubles).
 * Per walker: +w on rdm1[p,p] for every occupied p and on rdm2[tri(pq,pq)] for every occupied pair; a single h -> q with sign s adds
 * s w Re r to rdm1[q sorb + h] and, for every occupied k != h, s sigma w Re r to rdm2[tri(pair(h,k), pair(q,k))], sigma = -1 iff
 * (h > k) != (q > k); a double (h0 > h1 -> q0 > q1) adds s w Re r to rdm2[tri(pair(h0,h1), pair(q0,q1))].  A packed slot aliases (ij,kl)
 * with (kl,ij): it holds the Hermitian sum.  By construction dot(h1e, rdm1) + dot(h2e, rdm2) = sum_x w_x Re E_loc(x) for any integrals,
 * the diagonal of rdm1 sums to nele sum w and the diagonal pair slots of rdm2 to nele (nele - 1) / 2 sum w.
 * Walkers whose electron counts are not (noA, noB), or with bits at or above sorb, contribute nothing.
 *
 *   pynqs_rdm_scatter : any ansatz.  ratio: double[nbatch][ncomb] (is_complex: [nbatch][ncomb][2], the real part is used) in the column
 *        order of pynqs_comb (column 0 = x itself, not read).  ADDS into rdm1 / rdm2 (the caller zeroes them; several calls accumulate
 *        chunks of walkers) with f64 global atomics: NOT bit-reproducible.
 *   pynqs_rdm_rbm : real RBM (PYNQS_RBM_REAL), table from pynqs_rbm_table_build.  OVERWRITES rdm1 / rdm2.  Nothing of size
 *        nbatch x ncomb exists, no float atomics, every sum in a fixed order (walker order): two calls give the same bits.  workspace:
 *        pynqs_rdm_rbm_workspace bytes.  The amplitude ratio is (owner factor) x (lane constant) x prod_h (b_h + a_h g_h)
 *        (kernels_rdm.hip); the lane constant is exp(+-2 sum_o (sum_h W_ho - a_o)) over the two orbitals of the lane side, which must
 *        stay a finite double (|sum_h W_ho| below ~170 per orbital).
 *   pynqs_rdm_rbm_supported : 1 if the fused kernel serves (sorb even, (sorb / 2)^2 <= 2048, nhidden <= 512, its tables within 64 KiB of
 *        LDS), else 0: callers then use pynqs_rdm_scatter.
 *   pynqs_rdm_jrbm : Jastrow-RBM, psi(x) = exp(a.x + x^T M x) prod_h 2 cosh theta_h: pynqs_rdm_rbm's kernel in its Jastrow flavour, with
 *        pynqs_rdm_rbm's conventions (OVERWRITES, nbatch = 0 gives zeros, walkers with other electron counts are skipped, fixed order:
 *        two calls give the same bits).  rbm_table from pynqs_rbm_table_build, jastrow_table from pynqs_jastrow_table_build; workspace:
 *        pynqs_rdm_jrbm_workspace bytes = pynqs_rdm_rbm_workspace's + r [nbatch][sorb] doubles, r_o = sum_j S_oj x_j (S = M + M^T, zero
 *        diagonal).  The ratio gains exp(-2 sum_{i in F} x_i r_i + 4 sum_{i<j in F} S_ij x_i x_j) over the flipped orbitals F: the pair
 *        terms are constants of a workgroup and join the exponents that exist, exp(-+2 r_o) per orbital is staged once per walker; it
 *        must stay a finite double (2 sum_j |S_oj| below ~700).  tr M and the diagonal of M do not enter.  With M = 0 the result has the
 *        bits of pynqs_rdm_rbm.
 *   pynqs_rdm_jrbm_supported : pynqs_rdm_rbm_supported with 16 sorb more bytes of LDS.
 *   PYNQS_EINVAL, nothing launched, where _supported answers 0 or a pointer is null.                                                    */
int pynqs_rdm_scatter(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const double *w, const double *ratio,
                      int is_complex, double *rdm1, double *rdm2, void *stream);
int pynqs_rdm_rbm_supported(int sorb, int nele, int noA, int noB, int nhidden);
int64_t pynqs_rdm_rbm_workspace(int64_t nbatch, int sorb, int nhidden);
int pynqs_rdm_rbm(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const double *w, const void *rbm_table,
                  int nhidden, void *workspace, double *rdm1, double *rdm2, void *stream);
int pynqs_rdm_jrbm_supported(int sorb, int nele, int noA, int noB, int nhidden);
int64_t pynqs_rdm_jrbm_workspace(int64_t nbatch, int sorb, int nhidden);
int pynqs_rdm_jrbm(const uint64_t *bra, int64_t nbatch, int sorb, int nele, int noA, int noB, const double *w, const void *rbm_table,
                   const void *jastrow_table, int nhidden, void *workspace, double *rdm1, double *rdm2, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PYNQS_AMD_H */
