// Host-side constant dispatch: each helper turns one run-time value into a std::integral_constant and calls a generic lambda with it,
// so a launch site names its kernel once --
//     with_at_most<4, 8, 16>(C, [&](auto cr) { with_bool(ign, [&](auto ig) {
//         hipLaunchKernelGGL((focal_fwd_lean_kernel<cr(), ig()>), grid, block, 0, s, a); }); });
// -- and the kernel is instantiated for every value the helpers can yield.  A ladder that is NOT a full cross product keeps its
// subset with `if constexpr` inside the lambda (the discarded arm instantiates nothing; its else is no_instance()) or with an ordinary
// `if` in front of it.  with_view_set, which needs the CODES_* constants, is next to them in ptb_view_device.h.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "../../include/ptb_hip.h"

namespace ptb {

template <int V>
using int_c = std::integral_constant<int, V>;

// the else arm of an `if constexpr` that keeps a subset of the instances: the run-time values name a combination that is not compiled.
// Every call site's conditions rule it out, so reaching it is a bug in that site -- loud, never a launch that silently did not happen.
[[noreturn]] inline void no_instance(const char* kernel) {
    std::fprintf(stderr, "libptb_hip: no compiled instance of %s for this combination of arguments\n", kernel);
    std::abort();
}

template <class F>
void with_bool(bool b, F&& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// exact match; the last value is the fallback
template <int V0, int... Vs, class F>
void with_value(int v, F&& f) {
    if constexpr (sizeof...(Vs) == 0) f(int_c<V0>{});
    else if (v == V0) f(int_c<V0>{});
    else with_value<Vs...>(v, f);
}

// the first bucket that holds v; the last value is the fallback
template <int V0, int... Vs, class F>
void with_at_most(int v, F&& f) {
    if constexpr (sizeof...(Vs) == 0) f(int_c<V0>{});
    else if (v <= V0) f(int_c<V0>{});
    else with_at_most<Vs...>(v, f);
}

// element type of a source -> the kernels' LD parameter: 1 = fp32, 2 = fp16, 3 = bf16; a kernel whose parameter is the element type
// itself (IN) takes ld_dtype<ld()>()
template <class F>
void with_src_dtype(int dtype, F&& f) {
    if (dtype == PTB_F16) f(int_c<2>{});
    else if (dtype == PTB_BF16) f(int_c<3>{});
    else f(int_c<1>{});
}

// OPK: 0 = sum / mean, 1 = a non-linear reduction (the op is read at run time)
template <class F>
void with_reduction(int op, F&& f) {
    if (op >= PTB_RED_GMEAN) f(int_c<1>{});
    else f(int_c<0>{});
}
// ... with gmean, the common non-linear one, apart as 2 (branch-free)
template <class F>
void with_reduction3(int op, F&& f) {
    if (op == PTB_RED_GMEAN) f(int_c<2>{});
    else with_reduction(op, f);
}

// PTB_CROP_* kind of a merge+crop output; callers validate the kind first
template <class F>
void with_crop_kind(int kind, F&& f) {
    with_value<PTB_CROP_F32, PTB_CROP_U8, PTB_CROP_ARGMAX_U8, PTB_CROP_ARGMAX_I64, PTB_CROP_F16, PTB_CROP_BF16>(kind, f);
}

}  // namespace ptb
