// mx_dispatch.h — host side only: turns a run-time launch choice (lane-group width, operand kind, value type)
// into a template argument.  Every kernel that is templated on such a choice is launched through these helpers; a
// value outside the list given at the call is an error, never a silent default.
#pragma once
#include <type_traits>
#include "mx_common.h"

namespace mx {
#pragma GCC visibility push(hidden)

template <int... Vs> struct int_list {};
using lane_groups = int_list<4, 8, 16, 32, 64>;     // what pick_group(avg) can return

// f(std::integral_constant<int, V>{}) for the V of the list that equals v; f returns the call's status
template <int... Vs, typename F>
inline int dispatch_int(int_list<Vs...>, const char *what, const char *name, int v, F &&f)
{
    int rc = 0;
    const bool found = (... || (v == Vs && ((rc = f(std::integral_constant<int, Vs>{})), true)));
    return found ? rc : set_error("%s: unsupported %s %d", what, name, v);
}

// what the last launch_rows of this thread launched (mxd_last_row_launch; reporting only, set in api.hip)
void note_row_launch(const char *what, int G);

// One G-lane group per `rows_per_group` rows, `block` threads per block: launch(g, grid, block) holds the one
// hipLaunchKernelGGL of a kernel templated on g().
template <int... Gs, typename F>
inline int launch_rows(int_list<Gs...> groups, const char *what, int G, int64_t rows, int block, F &&launch,
                       int rows_per_group = 1)
{
    return dispatch_int(groups, what, "lane group", G, [&](auto g) {
        launch(g, dim3((unsigned)ceil_div(rows, (block / g()) * rows_per_group)), dim3((unsigned)block));
        MX_LAUNCH_CHECK();
        note_row_launch(what, g());
        return 0;
    });
}

// value type of a kernel templated on <VT, HAS_VALUES>
template <typename T, bool HAS> struct value_kind {
    using VT = T;
    static constexpr bool has_values = HAS;
};

template <typename F>
inline int dispatch_values(const char *what, int value_dtype, F &&f)
{
    switch (value_dtype) {
        case MX_F64: return f(value_kind<double, true>{});
        case MX_LGL: case MX_I32: return f(value_kind<int32_t, true>{});
        case MX_NONE: return f(value_kind<int32_t, false>{});
        default: return set_error("%s: unsupported value dtype %d", what, value_dtype);
    }
}

// element type of a dense operand: f(tag<double>{}) or f(tag<float>{}); the casts of its void pointers belong in f
template <typename T> struct tag { using type = T; };

template <typename F>
inline int dispatch_dense(const char *what, int dense_dtype, F &&f)
{
    switch (dense_dtype) {
        case MX_F64: return f(tag<double>{});
        case MX_F32: return f(tag<float>{});
        default: return set_error("%s: unsupported dense dtype %d", what, dense_dtype);
    }
}

#pragma GCC visibility pop
}  // namespace mx
