/* launch16.hpp -- the host-side pieces the estimator launchers (spectro16*.hip) share: helpers, not a framework.
   A launcher keeps its own order of refusals and early returns and calls these where it used to write the work out.
   Everything here is host arithmetic or a launch: no kernel is declared, changed or instantiated by this header. */
#ifndef GLFER_LAUNCH16_HPP
#define GLFER_LAUNCH16_HPP

#include <hip/hip_runtime.h>
#include <type_traits>
#include "spectro_params.h"

namespace glfer {
hipError_t allow_dynamic_lds(const void *kernel, size_t bytes);   // plan.h / glfer_hip.cpp: once per device, kernel and size class

/* Value dispatch: the run-time v as the one std::integral_constant<int, V> of the list that equals it, handed to f (which
   returns hipError_t); a value outside the list is hipErrorInvalidValue and f is not called.  Only the listed values are
   instantiated, so the list IS the set of kernels a ladder builds. */
template <int... Vs, class F>
static inline hipError_t with_value(int v, F &&f) {
  hipError_t e = hipErrorInvalidValue;
  (void)((v == Vs ? (e = f(std::integral_constant<int, Vs>{}), true) : false) || ...);
  return e;
}
/* the sample format of an argument block */
template <class F>
static inline hipError_t with_fmt(int fmt, F &&f) {
  return with_value<GLFER_FMT_F32, GLFER_FMT_S16, GLFER_FMT_U8>(fmt, static_cast<F &&>(f));
}

/* the hop in sixteenths of the block N = 2^L: 1..16, or 0 when it is no whole number of them */
template <int L>
static inline int hop_sixteenths(int H) {
  return (16 * H) % (1 << L) == 0 ? (16 * H) >> L : 0;
}

/* Persistent grids.  resident_workgroups: what the chip (256 CUs) holds of a kernel of `block` threads at `wps` wavefronts
   per SIMD.  persistent_grid: one workgroup per unit of work up to `cap` (the kernel's own multiple of the resident
   workgroups; a batch shares it among its streams), whole XCD slices from 64 up (xcd_block_index()). */
static inline long long resident_workgroups(int wps, int block) {
  const long long per_cu = (wps * 256) / block;
  return 256LL * (per_cu > 0 ? per_cu : 1);
}
static inline unsigned xcd_slices(unsigned grid) { return grid >= 64 ? grid & ~7u : grid; }
static inline unsigned persistent_grid(long long work, long long cap) { return xcd_slices((unsigned)(work < cap ? work : cap)); }

/* gridDim.y of a launch: the streams of its argument block (SpectroParams, IqParams, CrossParams) */
template <class P>
static inline unsigned batch_y(const P &p) { return p.nbatch > 1 ? (unsigned)p.nbatch : 1u; }
template <class P>
static inline dim3 batch_grid(unsigned grid, const P &p) { return dim3(grid, batch_y(p)); }

/* One launch: the kernel, its grid and block, dynamic LDS bytes, the stream, then the kernel's arguments (an argument block,
   or the submean kernels' plain list). */
template <class... KA, class... A>
static inline hipError_t launch(void (*kernel)(KA...), dim3 grid, dim3 block, size_t lds, hipStream_t st, const A &...args) {
  hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
  return hipGetLastError();
}
/* the same for a kernel whose dynamic LDS exceeds the default limit: the kernel it launches is the one it asks the limit for */
template <class... KA, class... A>
static inline hipError_t launch_dynamic_lds(void (*kernel)(KA...), dim3 grid, dim3 block, size_t lds, hipStream_t st, const A &...args) {
  const hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(kernel), lds);
  if (e != hipSuccess) return e;
  return launch(kernel, grid, block, lds, st, args...);
}
}  // namespace glfer
#endif
