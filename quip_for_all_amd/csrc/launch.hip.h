// Host launch layer: every kernel launch of the library goes through launch<Kern>() or launch_persistent<Kern>().
// The launch state of a kernel -- the dynamic-LDS limit configured on each device and, for persistent grids, the
// residency answer -- is a static of a function template over the kernel itself, so there is exactly one per kernel
// instantiation however many call sites launch it.
#pragma once
#include "quip_internal.h"

namespace quip {

template <auto Kern>
DynLdsCache& dyn_lds_state() {
  static DynLdsCache cache;
  return cache;
}
template <auto Kern>
ResidencyCache& residency_state() {
  static ResidencyCache cache;
  return cache;
}

// A kernel as a value, for a generic lambda that serves several instantiations: go(kernel_c<kern<1, 2>>) hands the
// kernel on to launch<decltype(k)::value>().
template <auto Kern>
struct KernelTag { static constexpr auto value = Kern; };
template <auto Kern>
constexpr KernelTag<Kern> kernel_c{};

// QUIP_OK / QUIP_ERR_LAUNCH
template <auto Kern, class... A>
int launch(dim3 grid, dim3 block, int lds, hipStream_t stream, A... args) {
  if (ensure_dyn_lds(dyn_lds_state<Kern>(), reinterpret_cast<const void*>(Kern), lds) != QUIP_OK) return QUIP_ERR_LAUNCH;
  hipLaunchKernelGGL(Kern, grid, block, lds, stream, args...);
  return hipGetLastError() == hipSuccess ? QUIP_OK : QUIP_ERR_LAUNCH;
}

// a grid whose workgroups spin on each other: QUIP_ERR_UNSUPPORTED unless all `nwg` of them are resident at once
template <auto Kern, class... A>
int launch_persistent(int nwg, int threads, int lds, hipStream_t stream, A... args) {
  if (ensure_dyn_lds(dyn_lds_state<Kern>(), reinterpret_cast<const void*>(Kern), lds) != QUIP_OK) return QUIP_ERR_LAUNCH;
  if (!persistent_grid_fits(residency_state<Kern>(), reinterpret_cast<const void*>(Kern), threads, lds, nwg))
    return QUIP_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(Kern, dim3(nwg), dim3(threads), lds, stream, args...);
  return hipGetLastError() == hipSuccess ? QUIP_OK : QUIP_ERR_LAUNCH;
}

}  // namespace quip
