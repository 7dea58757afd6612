// gs_launch.h -- host-side launch helpers shared by gs_kernels.hip and gs_masked.hip
#pragma once
#include <stdint.h>
#include <algorithm>
#include <type_traits>

namespace gs_detail {

// The field count F = 1 | 2 | 3 as a compile-time constant: calls
// fn(std::integral_constant<int, F>{}) and returns what it returns.  A launch
// inside a generic lambda reads
//   with_F(p->F, [&](auto f) { hipLaunchKernelGGL((k_x<decltype(f)::value>), ...); });
template <typename Fn>
inline auto with_F(int F, Fn&& fn) {
    if (F == 1) return fn(std::integral_constant<int, 1>{});
    if (F == 2) return fn(std::integral_constant<int, 2>{});
    return fn(std::integral_constant<int, 3>{});
}

// the two 32-bit words of a 64-bit seed, as the kernels take them
struct SeedWords {
    uint32_t lo, hi;
};
inline SeedWords seed_words(uint64_t seed) { return {(uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32)}; }

// workgroups of bs threads that cover n items: at least one, at most 2^20
inline unsigned nblk(long long n, int bs) {
    return (unsigned)std::max<long long>(1, std::min<long long>((n + bs - 1) / bs, 1 << 20));
}

}  // namespace gs_detail
