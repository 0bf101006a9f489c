// prover_selfcheck.hpp -- the Merkle self-check of a proof (zkhip_config.self_check): every plain layer of every tree of the proof against
// its children, the FRI leaves against the layers they hash, and the diagnostic text of what differs.  Included by prover.hip only (its
// last prove step, self_check_trees, hands over the trees and the FRI layers); tests/test_gpu_merkle_stress.py runs it.
#pragma once
#include <string.h>

#include <cstdio>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "poseidon2_coop.hpp"
#include "zkhip_internal.hpp"

namespace zk {

// every tree's digests as the previous proof left them
static std::mutex g_shadow_mu;
static std::map<const zkhip_tree*, std::vector<uint32_t>> g_shadow;
// the leaf digests of a FRI layer against the pairs they hash
__global__ __launch_bounds__(256) void k_check_pairs(const uint4* __restrict__ layer, size_t n_leaves, const uint32_t* __restrict__ digests, uint32_t* report) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_leaves) return;
    uint4 a = layer[2 * i], b = layer[2 * i + 1];
    uint32_t s[16] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, 0, 0, 0, 0, 0, 0, 0, 0};
    poseidon2_permute_rolled(s);
    bool same = true;
    for (int q = 0; q < 8; q++) same = same && s[q] == digests[i * 8 + q];
    if (!same) atomicAdd(&report[0], 1u), atomicMin(&report[1], (uint32_t)(i & 0xffffffu));
}

using NamedTrees = std::vector<std::pair<std::string, const zkhip_tree*>>;
struct FriLeaves {
    const uint32_t* layer;    // 2 * n_leaves ext
    const uint32_t* digests;  // the layer's tree: its leaf digests first
    size_t n_leaves;
};

// every differing node of the tree (first 8): what memory holds (read by copies, not kernels), what its stored children hash
// to, what the PREVIOUS proof of this key left in the node's place, and where else either value lies -- a lost store leaves
// the previous proof's node, a misdirected store puts the right node somewhere else, a foreign write leaves neither
static int self_check_describe(zkhip_ctx* ctx, const zkhip_tree* t, uint32_t* d_rep, std::string& bad) {
    hipStream_t st = ctx->stream;
    const unsigned lh = t->log_height;
    std::vector<uint32_t> all(merkle_digest_count(lh) * 8);
    ZK_HIP_CHECK(ctx, hipMemcpy(all.data(), t->d_digests, all.size() * 4, hipMemcpyDeviceToHost));
    std::vector<uint32_t> shadow;
    size_t shadow_first = 0;   // (first node of the shadow copy)
    {
        std::lock_guard<std::mutex> lk(g_shadow_mu);
        auto it = g_shadow.find(t);
        if (it != g_shadow.end()) shadow = it->second, shadow_first = merkle_digest_count(lh) - shadow.size() / 8;
    }
    auto words = [](const uint32_t* w) {
        char b[80];
        std::snprintf(b, sizeof b, "%08x %08x %08x %08x %08x %08x %08x %08x", w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]);
        return std::string(b);
    };
    auto where = [&](size_t node) {   // node number -> "layer l index i"
        unsigned l = 0;
        while (l < lh && node >= t->layer_off[l + 1]) l++;
        return "layer " + std::to_string(l) + " index " + std::to_string(node - t->layer_off[l]);
    };
    auto find_in = [&](const std::vector<uint32_t>& hay, size_t first_node, const uint32_t* w, size_t skip_node) {
        std::string r;
        for (size_t n = 0; n * 8 + 8 <= hay.size(); n++)
            if (n + first_node != skip_node && memcmp(&hay[n * 8], w, 32) == 0) r += (r.empty() ? "" : ", ") + where(n + first_node);
        return r.empty() ? std::string("nowhere") : r;
    };
    unsigned shown = 0;
    for (unsigned l = 1; l <= lh && shown < 8; l++) {
        const unsigned level = lh - l;
        if (level < t->level_cnt.size() && t->level_cnt[level]) continue;
        for (size_t idx = 0; idx < ((size_t)1 << level) && shown < 8; idx++) {
            uint32_t kids[16];
            memcpy(kids, &all[(t->layer_off[l - 1] + 2 * idx) * 8], 64);
            poseidon2_permute_host(kids);
            const size_t node = t->layer_off[l] + idx;
            const uint32_t* stored = &all[node * 8];
            if (memcmp(kids, stored, 32) == 0) continue;
            shown++;
            unsigned diff_mask = 0;
            for (int q = 0; q < 8; q++) diff_mask |= (stored[q] != kids[q]) << q;
            char head[200];
            std::snprintf(head, sizeof head, "{node layer %u index %zu (byte offset 0x%zx in the store, device address %p) words differing: 0x%02x; ", l, idx, node * 32,
                          (const void*)(t->d_digests + node * 8), diff_mask);
            bad += head;
            bad += "stored [" + words(stored) + "]; children hash to [" + words(kids) + "]; ";
            if (!shadow.empty() && node >= shadow_first) {
                const uint32_t* prevw = &shadow[(node - shadow_first) * 8];
                bad += "previous proof had [" + words(prevw) + "] there: " + (memcmp(prevw, stored, 32) == 0 ? "THE SAME (a store that did not land)" : "different") + "; ";
                bad += "the stored value lies in the previous proof's store at: " + find_in(shadow, shadow_first, stored, (size_t)-1) + "; ";
            } else {
                bad += "no copy of the previous proof's node; ";
            }
            bad += "the stored value lies elsewhere in this store at: " + find_in(all, 0, stored, node) + "; the right value lies elsewhere at: " + find_in(all, 0, kids, node) + "} ";
        }
    }
    uint32_t again[2] = {0, 0xffffffffu};
    ZK_HIP_CHECK(ctx, hipMemcpy(d_rep, again, 8, hipMemcpyHostToDevice));
    ZK_TRY(merkle_check_tree(ctx, t, d_rep));
    ZK_HIP_CHECK(ctx, hipStreamSynchronize(st));
    ZK_HIP_CHECK(ctx, hipMemcpy(again, d_rep, 8, hipMemcpyDeviceToHost));
    bad += "[the host finds " + std::to_string(shown) + " differing nodes in the copy; a second device check finds " + std::to_string(again[0]) + "] ";
    return ZKHIP_OK;
}

// diagnosis: every plain layer of every tree of this proof against its children, the FRI leaves against the layers they hash
static int self_check_run(zkhip_ctx* ctx, const NamedTrees& trees, const std::vector<FriLeaves>& fri) {
    hipStream_t st = ctx->stream;
    const size_t n_rep = trees.size() + fri.size();
    std::vector<uint32_t> rep(2 * n_rep);
    for (size_t i = 0; i < n_rep; i++) rep[2 * i] = 0, rep[2 * i + 1] = 0xffffffffu;
    uint32_t* d_rep = nullptr;
    ZK_HIP_CHECK(ctx, hipMalloc(&d_rep, rep.size() * 4));
    ZK_HIP_CHECK(ctx, hipMemcpyAsync(d_rep, rep.data(), rep.size() * 4, hipMemcpyHostToDevice, st));
    ZK_HIP_CHECK(ctx, hipStreamSynchronize(st));
    for (size_t i = 0; i < trees.size(); i++) ZK_TRY(merkle_check_tree(ctx, trees[i].second, d_rep + 2 * i));
    for (size_t l = 0; l < fri.size(); l++)
        hipLaunchKernelGGL(k_check_pairs, dim3((unsigned)((fri[l].n_leaves + 255) / 256)), dim3(256), 0, st, (const uint4*)fri[l].layer, fri[l].n_leaves,
                           fri[l].digests, d_rep + 2 * (trees.size() + l));
    ZK_HIP_CHECK(ctx, hipMemcpyAsync(rep.data(), d_rep, rep.size() * 4, hipMemcpyDeviceToHost, st));
    ZK_HIP_CHECK(ctx, hipStreamSynchronize(st));
    std::string bad;
    for (size_t i = 0; i < trees.size(); i++)
        if (rep[2 * i]) ZK_TRY(self_check_describe(ctx, trees[i].second, d_rep, bad));
    (void)hipFree(d_rep);
    for (size_t i = 0; i < trees.size(); i++) {   // what this proof leaves, for the next one's diagnosis
        const zkhip_tree* t = trees[i].second;
        // (the tail of the store: the layers of <= 2^13 nodes -- all the fused kernels' layers; a large tree's whole store would take longer than the proof)
        const size_t total = merkle_digest_count(t->log_height), keep = std::min(total, ((size_t)2 << 13) - 1);
        std::vector<uint32_t> copy(keep * 8);
        ZK_HIP_CHECK(ctx, hipMemcpy(copy.data(), t->d_digests + (total - keep) * 8, copy.size() * 4, hipMemcpyDeviceToHost));
        std::lock_guard<std::mutex> lk(g_shadow_mu);
        g_shadow[t].swap(copy);
    }
    for (size_t i = 0; i < n_rep; i++)
        if (rep[2 * i]) {
            const std::string name = i < trees.size() ? "tree " + trees[i].first + " (height 2^" + std::to_string(trees[i].second->log_height) + ")"
                                                      : "leaves of fri " + std::to_string(i - trees.size());
            bad += name + ": " + std::to_string(rep[2 * i]) + " nodes differ from the hash of their children, first layer " + std::to_string(rep[2 * i + 1] >> 24) +
                   " index " + std::to_string(rep[2 * i + 1] & 0xffffffu) + "; ";
        }
    if (!bad.empty()) {
        std::fprintf(stderr, "[zkhip self-check] %s\n", bad.c_str());
        return set_error(ctx, ZKHIP_ERR_HIP, "self-check: " + bad);
    }
    return ZKHIP_OK;
}

}  // namespace zk
