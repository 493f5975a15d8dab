#pragma once
// Host-side rules every batched entry over host tables follows (api_batch.cpp, api_merkle_batch.cpp, api_mle_batch.cpp): the
// range check of u64 field values, their narrowing to u32, the 16-byte packing of the narrowed tables, and the order in which a
// batch reports errors.  Plain C++, no HIP: compiled into the CPU driver tests/c_driver/sumcheck_verify_host.cpp through
// sumcheck_verify_host.hpp, like open_plan.hpp and verify_plan.hpp into theirs.
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "zigz_hip.h"

namespace zk {

// all n values are canonical BabyBear elements (< p)
inline bool canonical(const uint64_t *v, size_t n) {
    for (size_t j = 0; j < n; j++)
        if (v[j] >= ZIGZ_BABYBEAR_P) return false;
    return true;
}
// u64 -> packed u32; false at the first value >= p
inline bool narrow(const uint64_t *src, size_t n, uint32_t *dst) {
    for (size_t j = 0; j < n; j++) {
        if (src[j] >= ZIGZ_BABYBEAR_P) return false;
        dst[j] = (uint32_t)src[j];
    }
    return true;
}
// k tables of ns[i] u32 words packed one behind the other, every table 16-byte aligned: table i starts at word at[i], at[k]
// words in all
inline std::vector<size_t> packed_offsets(const size_t *ns, size_t k) {
    std::vector<size_t> at(k + 1, 0);
    for (size_t i = 0; i < k; i++) at[i + 1] = at[i] + ((ns[i] + 3) & ~(size_t)3);
    return at;
}
// A host form's checks before anything is uploaded.  check(&f) runs the checks that do not read the tables' values, pair by
// pair, and returns the first failure's status with f = its pair.  The single calls, made in order, would have stopped at a
// table BEFORE pair f that holds a value >= p: such a table is reported instead (ZIGZ_ERR_NOT_CANONICAL; *value_found says so).
// When every pair passes, the caller checks the values while it narrows them.  f left at k: the failure is not about one pair.
template <class Check>
zigz_status checks_in_call_order(const uint64_t *const *tables, const size_t *ns, size_t k, size_t *bad_index, Check check,
                                 bool *value_found = nullptr) {
    size_t f = k;
    zigz_status st = check(&f);
    bool value = false;
    if (st != ZIGZ_OK && f < k) {
        for (size_t i = 0; i < f && !value; i++)
            if (!canonical(tables[i], ns[i])) {
                value = true;
                f = i;
                st = ZIGZ_ERR_NOT_CANONICAL;
            }
        if (bad_index) *bad_index = f;
    }
    if (value_found) *value_found = value;
    return st;
}

}  // namespace zk
