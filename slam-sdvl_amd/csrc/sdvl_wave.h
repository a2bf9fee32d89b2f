// sdvl_wave.h — the wave64 primitives that more than one kernel file uses.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace {

// LDS hand-off between the lanes of ONE wave: order the compiler's view of memory, no s_barrier needed (the lanes of a wave execute
// their LDS instructions in order)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// sum over the 64 lanes (all active), result in every lane: data-parallel-primitive adds inside the 16-lane rows, two row
// broadcasts, one readlane — 7 VALU instructions instead of 6 x (ds_bpermute + add) with their address arithmetic
__device__ __forceinline__ int wave_sum_i32(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);  // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);  // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xe, false);  // row_shr:4, banks 1-3
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xc, false);  // row_shr:8, banks 2-3: lane 15 of a row holds the row's sum
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);  // row_bcast:15 into rows 1 and 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);  // row_bcast:31 into rows 2 and 3: lane 63 holds the total
  return __builtin_amdgcn_readlane(v, 63);
}

// minimum over the 64 lanes (all active) in every lane: DPP steps inside the 16-lane rows, two row broadcasts, one readlane
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
  const auto step = [](uint32_t x, auto ctrl, auto rows) {
    const uint32_t o = static_cast<uint32_t>(__builtin_amdgcn_update_dpp(-1, static_cast<int>(x), decltype(ctrl)::value, decltype(rows)::value, 0xf, false));
    return o < x ? o : x;
  };
  v = step(v, std::integral_constant<int, 0x111>{}, std::integral_constant<int, 0xf>{});  // row_shr:1
  v = step(v, std::integral_constant<int, 0x112>{}, std::integral_constant<int, 0xf>{});  // row_shr:2
  v = step(v, std::integral_constant<int, 0x114>{}, std::integral_constant<int, 0xf>{});  // row_shr:4
  v = step(v, std::integral_constant<int, 0x118>{}, std::integral_constant<int, 0xf>{});  // row_shr:8: lane 15 of a row holds the row's minimum
  v = step(v, std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xa>{});  // row_bcast:15 into rows 1 and 3
  v = step(v, std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xc>{});  // row_bcast:31 into rows 2 and 3
  return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), 63));
}

// the same for floats: lanes without a source add 0.0f, every lane gets the same bits
#define SDVL_DPP_F32(x, ctrl, rows, banks) \
  __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), ctrl, rows, banks, false))
__device__ __forceinline__ float wave_sum_dpp_f32(float x) {
  x += SDVL_DPP_F32(x, 0x111, 0xf, 0xf);
  x += SDVL_DPP_F32(x, 0x112, 0xf, 0xf);
  x += SDVL_DPP_F32(x, 0x114, 0xf, 0xe);
  x += SDVL_DPP_F32(x, 0x118, 0xf, 0xc);
  x += SDVL_DPP_F32(x, 0x142, 0xa, 0xf);
  x += SDVL_DPP_F32(x, 0x143, 0xc, 0xf);
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 63));
}
#undef SDVL_DPP_F32

}  // namespace
