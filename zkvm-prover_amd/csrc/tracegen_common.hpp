// tracegen_common.hpp -- what the trace generators' host sides share: the conversion of count tables out of Montgomery form and back
// around a generator's increments, the kernels' check of a record word, the launch frame every generator with a device counter runs in, and
// the per-chip cache of AIR programs.
#pragma once
#include <initializer_list>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/zkhip_air.hpp"
#include "babybear.hpp"
#include "zkhip_internal.hpp"

namespace zk {

struct TableRef {
    uint32_t* d;
    size_t words;
};
// integer counts <-> Montgomery counts, one launch on the context's stream (tracegen.hip: k_table_repr).  Counts stay far below p: at
// most 2^27 rows x a few hundred columns per call, and the sum is reduced mod p, which is what the bus argument needs anyway.
void table_repr(zkhip_ctx* ctx, uint32_t* d, size_t words, bool to_monty);
// the same for the tables a generator counts into; nothing where the caller keeps them canonical (zkhip_tables_canonical)
inline void tables_repr(zkhip_ctx* ctx, std::initializer_list<TableRef> tabs, bool to_monty) {
    if (ctx->tables_canonical) return;
    for (const TableRef& t : tabs) table_repr(ctx, t.d, t.words, to_monty);
}

// a record word on the device: refused (counted, and read as 0) unless it is a field element; returns Montgomery form
__device__ __forceinline__ uint32_t field_word(uint32_t v, uint32_t* bad) {
    if (v >= P) atomicAdd(bad, 1u), v = 0;
    return to_monty(v);
}

// the range (or, one column further, XOR) multiplicities of the 8-bit table
constexpr size_t BITWISE_WORDS = (size_t)1 << 16;

// n records fit N rows, and the tuple table covers the chip's carries (min_y = 0: the chip has no tuple table)
inline int tracegen_shape(zkhip_ctx* ctx, const std::string& name, size_t n, size_t N, uint32_t size_x, uint32_t size_y, uint32_t min_y) {
    if (n > N) return set_error(ctx, ZKHIP_ERR_INVALID, name + ": more records than rows");
    if (min_y && (size_x < 256 || size_y < min_y || (size_t)size_x * size_y > ((size_t)1 << 27)))
        return set_error(ctx, ZKHIP_ERR_INVALID, name + ": the tuple table must cover (x < 256, y < " + std::to_string(min_y) + ")");
    return ZKHIP_OK;
}

// a launch callback's status: one that returns nothing has issued kernels only, and those are checked by the frame
template <class Launch>
int tracegen_launch(Launch& launch, uint32_t* bad) {
    if constexpr (std::is_void_v<decltype(launch(bad))>) {
        launch(bad);
        return ZKHIP_OK;
    } else {
        return launch(bad);
    }
}

// One generator call under the profile scope `name`: the device counter of refused records, the tables out of Montgomery form,
// launch(bad) for the generator's kernels (and memsets: a callback that can fail returns its status), the tables back, and the verdict
// (`refusal` names what the kernels refuse).  The order is what the deferred checks rely on: the counter before the scope, the tables
// back before the error check, the verdict last.
template <class Launch>
int tracegen_frame(zkhip_ctx* ctx, const char* name, std::initializer_list<TableRef> tabs, Launch&& launch, const std::string& refusal) {
    void* flag = nullptr;
    ZK_TRY(tracegen_flag(ctx, &flag));
    KernelScope ks(ctx, name);
    tables_repr(ctx, tabs, false);
    ZK_TRY(tracegen_launch(launch, (uint32_t*)flag));
    tables_repr(ctx, tabs, true);
    ZK_HIP_CHECK(ctx, hipGetLastError());
    return tracegen_finish(ctx, flag, refusal);
}

// The frame of a generator whose whole trace is the count table: counted from zero, or (accumulate) on top of what the table holds
template <class Launch>
int tracegen_count_frame(zkhip_ctx* ctx, const char* name, TableRef tab, int accumulate, Launch&& launch, const std::string& refusal) {
    return tracegen_frame(
        ctx, name, {},
        [&](uint32_t* bad) -> int {
            if (!accumulate) ZK_HIP_CHECK(ctx, hipMemsetAsync(tab.d, 0, tab.words * 4, ctx->stream));
            else tables_repr(ctx, {tab}, false);
            ZK_TRY(tracegen_launch(launch, bad));
            tables_repr(ctx, {tab}, true);
            return ZKHIP_OK;
        },
        refusal);
}

// AIR programs of one chip by key (modulus, buses, ...), built at first use and kept for the life of the process: the zkhip_air handed
// out points into the cache
template <class Key>
struct AirCache {
    std::mutex mu;
    std::map<Key, std::vector<uint32_t>> programs;
    template <class Build>
    int get(const Key& key, size_t width, Build&& build, zkhip_air* out) {
        try {
            std::lock_guard<std::mutex> lk(mu);
            auto it = programs.find(key);
            if (it == programs.end()) {
                zkhip::air::AirBuilder b(width, 0);
                build(b);
                it = programs.emplace(key, b.program()).first;
            }
            out->program = it->second.data(), out->program_len = it->second.size(), out->log_height = 0, out->width = width, out->n_pvs = 0;
            out->prep_trace = nullptr, out->prep_commit = nullptr;
        } catch (const std::exception&) {
            return ZKHIP_ERR_INVALID;
        }
        return ZKHIP_OK;
    }
};

}  // namespace zk
