// Temporary storage of rocPRIM's device-wide radix sorts over all bits of the key: size queries, no kernel is launched.  A query
// costs microseconds and calls that run once per batch ask for the same sizes again and again, so every query shape (key type,
// value type) remembers its last four answers.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

namespace tpnet {

struct SizeMemo {
    size_t n[4] = {0, 0, 0, 0}, v[4] = {0, 0, 0, 0};
    int next = 0;
    template <class Query> size_t operator()(size_t count, Query query) {
        for (int i = 0; i < 4; ++i)
            if (v[i] && n[i] == count) return v[i];
        const int i = next++ & 3;
        n[i] = count;
        return v[i] = query();
    }
};

template <class K, class V> static size_t sort_pairs_tmp(size_t n) {
    static thread_local SizeMemo memo;
    return memo(n, [n] {
        size_t b = 0;
        (void)rocprim::radix_sort_pairs(nullptr, b, (K*)nullptr, (K*)nullptr, (V*)nullptr, (V*)nullptr, n, 0, 8 * sizeof(K),
                                        (hipStream_t)0, false);
        return b;
    });
}
template <class K> static size_t sort_keys_tmp(size_t n) {
    static thread_local SizeMemo memo;
    return memo(n, [n] {
        size_t b = 0;
        (void)rocprim::radix_sort_keys(nullptr, b, (K*)nullptr, (K*)nullptr, n, 0, 8 * sizeof(K), (hipStream_t)0, false);
        return b;
    });
}

}  // namespace tpnet
