// tracegen_common.hpp -- what the trace generators' host sides share: the conversion of count tables out of Montgomery form and back
// around a generator's increments, the launch frame of the limb chips, and the per-chip cache of AIR programs.
#pragma once
#include <initializer_list>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/zkhip_air.hpp"
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

// the range (or, one column further, XOR) multiplicities of the 8-bit table
constexpr size_t BITWISE_WORDS = (size_t)1 << 16;

// n records fit N rows, and the tuple table covers the chip's carries (min_y = 0: the chip has no tuple table)
inline int tracegen_shape(zkhip_ctx* ctx, const std::string& name, size_t n, size_t N, uint32_t size_x, uint32_t size_y, uint32_t min_y) {
    if (n > N) return set_error(ctx, ZKHIP_ERR_INVALID, name + ": more records than rows");
    if (min_y && (size_x < 256 || size_y < min_y || (size_t)size_x * size_y > ((size_t)1 << 27)))
        return set_error(ctx, ZKHIP_ERR_INVALID, name + ": the tuple table must cover (x < 256, y < " + std::to_string(min_y) + ")");
    return ZKHIP_OK;
}

// One generator call under the profile scope `name`: the tables out of Montgomery form, launch(bad) for the trace kernel with the device
// counter of refused records, the tables back, and the verdict (`refusal` names what the kernel refuses).
template <class Launch>
int tracegen_frame(zkhip_ctx* ctx, const char* name, std::initializer_list<TableRef> tabs, Launch&& launch, const std::string& refusal) {
    void* flag = nullptr;
    ZK_TRY(tracegen_flag(ctx, &flag));
    KernelScope ks(ctx, name);
    tables_repr(ctx, tabs, false);
    launch((uint32_t*)flag);
    tables_repr(ctx, tabs, true);
    ZK_HIP_CHECK(ctx, hipGetLastError());
    return tracegen_finish(ctx, flag, refusal);
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
