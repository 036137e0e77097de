// ldpc_layer_plan.h -- host planner of the block-parallel layered decode (kernel: ldpc_layered_block.hip).
//
// Pure integer C++17 on host vectors, in the style of ldpc_plan.h: the validation of a layer partition
// (layer_partition_error), and the geometry and tables of one decoder (layer_plan).  Nothing here knows a device: the
// tables come back as host data, the engine uploads them, and a host test drives the planner in a process of its own.
//
// A layer is a run of consecutive checks in CSR order whose variable sets are pairwise disjoint, so the kernel updates
// all of them at once: thread (g, j) of a workgroup owns check j of the current layer for codeword g.
//
// LDS of one codeword (dword offsets inside its row of `row_words` dwords, an ODD number so that one variable of
// different codewords falls in different banks):
//   [0, n)                        fp32 posteriors, variable v at dword v
//   min-sum forms, from rec_off:  the check records, one array per field so that the lanes of a layer step touch
//                                 consecutive dwords: m1[m], m2[m], sign words [W][m], arg-min words [W][m]
//                                 (W = 1 up to 32 edges per check, 2 up to kBlkMaxDeg = 64: the record format's widest check)
//   RCQ, from rec_off:            one code byte (level | sign << 7) per PLAN ENTRY, at the entry's index
// After the G rows: the workgroup's bookkeeping words (layer_flag_words).
//
// Plan entries: layer l holds S_l checks whose widest has D_l edges; edge k of its check j is entry
// entry_base[l] + k * S_l + j ("layer-transposed": the lanes of a layer step read consecutive entries).  An entry beyond
// its check's degree is a hole (kBlkHole) that nothing reads.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "ldpc_resident_geom.h"

namespace ldpc {

constexpr int kBlkMaxDeg = 64;                 // widest check of the record format (two 32-bit words of sign / arg-min bits)
constexpr int kBlkMaxThreads = 512;            // workgroup size limit of layered_block_lds (its __launch_bounds__)
constexpr uint32_t kBlkHole = 0xffffffffu;
enum { kBlkMinSum = 0, kBlkRcq = 1 };

// bookkeeping words after the codeword rows: per codeword { unsatisfied, frozen, iterations }, then the live count
inline size_t layer_flag_words(int G) { return 3 * (size_t)G + 1; }

// "" when layer_ptr [n_layers + 1] is a partition of the m checks into runs of variable-disjoint checks, else what is
// wrong with it (naming the layer, and the variable two of its checks share)
inline std::string layer_partition_error(int n, int m, const int32_t *check_ptr, const int32_t *var_idx, int n_layers,
                                         const int32_t *layer_ptr)
{
    char buf[192];
    if (n_layers < 1 || !layer_ptr) return "layer_ptr is missing (n_layers must be >= 1)";
    if (layer_ptr[0] != 0 || layer_ptr[n_layers] != m) {
        snprintf(buf, sizeof(buf), "layer_ptr must span [0, m = %d], got %d .. %d", m, layer_ptr[0], layer_ptr[n_layers]);
        return buf;
    }
    for (int l = 0; l < n_layers; ++l)
        if (layer_ptr[l + 1] <= layer_ptr[l] || layer_ptr[l + 1] > m) {
            snprintf(buf, sizeof(buf), "layer_ptr is not strictly ascending at layer %d", l);
            return buf;
        }
    std::vector<int> stamp((size_t)std::max(n, 1), -1);
    for (int l = 0; l < n_layers; ++l)
        for (int e = check_ptr[layer_ptr[l]]; e < check_ptr[layer_ptr[l + 1]]; ++e) {
            const int v = var_idx[e];
            if (stamp[v] == l) {
                snprintf(buf, sizeof(buf), "layer %d (checks %d .. %d) is not variable-disjoint: variable %d is in two of its checks",
                         l, layer_ptr[l], layer_ptr[l + 1] - 1, v);
                return buf;
            }
            stamp[v] = l;
        }
    return "";
}

struct LayerPlan {
    bool ok = false;
    std::string why;               // why the code does not qualify (ok == false)
    int n = 0, m = 0, L = 0, kind = kBlkMinSum;
    int W = 1;                     // 32-bit mask words per check record (min-sum forms)
    int G = 0, lpc = 0, threads = 0;   // codewords per workgroup, lanes per codeword, workgroup size (a multiple of 64)
    int max_layer = 0, entries = 0;
    unsigned row_words = 0, rec_off = 0;
    size_t lds_bytes = 0;
    std::vector<int> layer_ptr, entry_base;     // [L + 1]
    std::vector<int> deg;                       // [m]
    std::vector<uint32_t> off;                  // [entries] byte offset (4 * variable) of the entry's posterior in the row; kBlkHole
    std::vector<int> edge_of_entry;             // [entries] CSR edge id, -1: hole
};

// geometry and tables for a VALID partition (layer_partition_error == "") of a valid CSR
inline LayerPlan layer_plan(int n, int m, const int32_t *check_ptr, const int32_t *var_idx, int n_layers,
                            const int32_t *layer_ptr, int kind)
{
    LayerPlan p;
    p.n = n; p.m = m; p.L = n_layers; p.kind = kind;
    char buf[160];
    if (n_layers < 1) { p.why = "the graph declares no layers"; return p; }
    if (m < 1 || check_ptr[m] < 1) { p.why = "the graph has no edges"; return p; }
    int max_dc = 0;
    p.deg.resize(m);
    for (int i = 0; i < m; ++i) { p.deg[i] = check_ptr[i + 1] - check_ptr[i]; max_dc = std::max(max_dc, p.deg[i]); }
    if (max_dc > kBlkMaxDeg) {
        snprintf(buf, sizeof(buf), "check degree %d exceeds the check record's %d edges", max_dc, kBlkMaxDeg);
        p.why = buf;
        return p;
    }
    p.W = max_dc > 32 ? 2 : 1;
    p.layer_ptr.assign(layer_ptr, layer_ptr + n_layers + 1);
    p.entry_base.assign((size_t)n_layers + 1, 0);
    long long entries = 0;
    for (int l = 0; l < n_layers; ++l) {
        const int c0 = layer_ptr[l], S = layer_ptr[l + 1] - c0;
        int D = 0;
        for (int j = 0; j < S; ++j) D = std::max(D, p.deg[c0 + j]);
        p.max_layer = std::max(p.max_layer, S);
        p.entry_base[l] = (int)entries;
        entries += (long long)S * D;
        if (entries > (1ll << 30)) { p.why = "the layer plan exceeds 2^30 entries"; return p; }
    }
    p.entry_base[n_layers] = (int)entries;
    p.entries = (int)entries;
    p.off.assign((size_t)entries, kBlkHole);
    p.edge_of_entry.assign((size_t)entries, -1);
    for (int l = 0; l < n_layers; ++l) {
        const int c0 = layer_ptr[l], S = layer_ptr[l + 1] - c0;
        for (int j = 0; j < S; ++j)
            for (int k = 0; k < p.deg[c0 + j]; ++k) {
                const size_t at = (size_t)p.entry_base[l] + (size_t)k * S + j;
                const int e = check_ptr[c0 + j] + k;
                p.off[at] = (uint32_t)var_idx[e] * 4u;
                p.edge_of_entry[at] = e;
            }
    }
    // one codeword's row: posteriors, then records (min-sum) or code bytes (RCQ); an odd number of dwords
    p.rec_off = (unsigned)n;
    const unsigned long long tail = kind == kBlkMinSum ? (unsigned long long)(2 + 2 * p.W) * (unsigned long long)m
                                                       : ((unsigned long long)entries + 3) / 4;
    unsigned long long words = (unsigned long long)n + tail;
    words |= 1ull;
    if (words * 4 + layer_flag_words(1) * 4 > kLdsBytes) {
        snprintf(buf, sizeof(buf), "one codeword's state (%llu bytes) does not fit %zu bytes of LDS", words * 4, kLdsBytes);
        p.why = buf;
        return p;
    }
    p.row_words = (unsigned)words;
    // codewords per workgroup: what LDS holds -- half of it when that still leaves eight, so that two workgroups share
    // a CU and one's barrier waits overlap the other's work; lanes per codeword: the widest layer, as the thread limit allows
    const size_t row_bytes = (size_t)words * 4;
    auto fits = [&](int G) { return (size_t)G * row_bytes + layer_flag_words(G) * 4; };
    int g_full = (int)std::min<size_t>(kLdsBytes / row_bytes, (size_t)kBlkMaxThreads);
    while (g_full > 1 && fits(g_full) > kLdsBytes) --g_full;
    int G = g_full >= 8 ? g_full / 2 : g_full;
    while (G > 1 && fits(G) > (g_full >= 8 ? kLdsBytes / 2 : kLdsBytes)) --G;
    const int lpc = std::min(p.max_layer, kBlkMaxThreads);
    G = std::max(1, std::min(G, kBlkMaxThreads / lpc));
    p.G = G;
    p.lpc = lpc;
    p.threads = (G * lpc + 63) / 64 * 64;
    p.lds_bytes = fits(G);
    p.ok = true;
    return p;
}

}  // namespace ldpc
