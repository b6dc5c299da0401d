// ss_common.h -- what the table-driven SAMPLE_SPACE local-energy kernels share: the column-major ones (kernels_eloc.hip) and the
// key-major one (kernels_eloc_keys.hip).  Device side: the spin-flip partner of a determinant, psi of a table entry, the store of
// psi(x).  Host side: the argument checks, the division by psi(x) after a chunked launch, bool -> template-parameter dispatch and
// the launch with dynamic LDS.
#pragma once

#include <type_traits>

#include "detcore.h"
#include "launch.h"
#include "plan.h"

namespace pynqs {

// Spin-flip partner of a determinant (vmc/energy/flip.py:322-418, utils/public_function.py:966-1007): alpha <-> beta occupations
// exchanged in place (orbitals 2k <-> 2k + 1 live in the same word); returns true if eta_m = (-1)^(doubly occupied spatial orbitals)
// is -1 (the same for a determinant and its partner).
template <int LEN>
__device__ __forceinline__ bool spin_flip_ket(uint64_t (&ket)[LEN]) {
  uint32_t pairs = 0;
#pragma unroll
  for (int i = 0; i < LEN; ++i) {
    const uint64_t w = ket[i];
    pairs += (uint32_t)__popcll(w & (w >> 1) & 0x5555555555555555ull);
    ket[i] = ((w >> 1) & 0x5555555555555555ull) | ((w & 0x5555555555555555ull) << 1);
  }
  return pairs & 1u;
}

// psi of table entry pos (one 16-byte load when complex: the column-major kernels are bound by the number of vector-memory
// instructions, TD busy 91 %), 0 if pos < 0
template <bool CPLX>
__device__ __forceinline__ void table_value(const double *__restrict__ wf, int64_t pos, double &vr, double &vi) {
  vr = 0.0; vi = 0.0;
  if (pos >= 0) {
    if constexpr (CPLX) {
      typedef double d2 __attribute__((ext_vector_type(2)));
      const d2 v = *reinterpret_cast<const d2 *>(wf + 2 * pos);
      vr = v[0]; vi = v[1];
    } else vr = wf[pos];
  }
}

// psi(x) goes to the walker's slot, unless this is the flip pass (psi0 is its input)
template <bool CPLX>
__device__ __forceinline__ void store_psi0(double *__restrict__ slot, double vr, double vi, bool flip) {
  if (!flip) {
    slot[0] = vr;
    if constexpr (CPLX) slot[1] = vi;
  }
}

// =================================================================================================
// host side

// the checks every SAMPLE_SPACE launch starts with
static inline int eloc_common_checks(int sorb, int nele, int noA, int noB, int64_t nbatch, int64_t nkeys, SDParams *p, PlanLayout *pl) {
  if (!make_sd_params(sorb, nele, noA, noB, p)) return set_error(PYNQS_EINVAL, "bad sorb/noA/noB");
  if (!make_plan_layout(sorb, pl)) return set_error(PYNQS_EINVAL, "plan needs an even sorb in [2, 192]");
  if (nbatch < 0 || nbatch > 0x7fffffffll) return set_error(PYNQS_EINVAL, "bad nbatch");
  if (nkeys < 0) return set_error(PYNQS_EINVAL, "bad nkeys");
  return PYNQS_OK;
}

// eloc = acc / psi0 in place on acc (complex division when cplx): what follows a launch whose workgroups added partial sums
// (eloc_divide_kernel, kernels_eloc.hip)
void eloc_divide(double *acc, const double *psi0, int64_t nbatch, bool cplx, hipStream_t st);

// a run-time bool as a template parameter: f(std::true_type / std::false_type)
template <typename F>
static inline int with_bool(bool b, F &&f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}

// launch with `lds` bytes of dynamic LDS (above 64 KiB a kernel has to be told)
template <typename Kernel, typename... Args>
static inline int ss_launch(Kernel kernel, uint32_t grid, uint32_t threads, size_t lds, hipStream_t st, Args... args) {
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return check_launch("hipFuncSetAttribute");
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds, st, args...);
  return PYNQS_OK;
}

}  // namespace pynqs
