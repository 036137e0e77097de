// Stand-alone driver of the block-parallel layered decode's planner (csrc/ldpc_layer_plan.h), built by
// tests/test_layer_plan_host.py with g++ and the address / undefined-behaviour sanitizers and run as a process of its own.
//
//   layer_plan_shim <in> <out>
// in : "n m E L kind", then check_ptr [m + 1], var_idx [E], layer_ptr [L + 1] (one line each)
// out: one line per table, "name count v0 v1 ..."; for an invalid partition the single line "partition_error <text>", for a
//      code that does not qualify "ok 1 0" and "why <text>"
#include <cstdio>
#include <fstream>
#include <iostream>
#include <vector>

#include "ldpc_layer_plan.h"

template <typename V>
static void put(std::ofstream &out, const char *name, const V &v)
{
    out << name << ' ' << v.size();
    for (const auto &x : v) out << ' ' << (long long)x;
    out << '\n';
}

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s <in> <out>\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    int n, m, E, L, kind;
    if (!(in >> n >> m >> E >> L >> kind)) return 3;
    std::vector<int32_t> cp((size_t)m + 1), vi((size_t)E), lp((size_t)L + 1);
    for (auto &x : cp) in >> x;
    for (auto &x : vi) in >> x;
    for (auto &x : lp) in >> x;
    if (!in) return 3;
    std::ofstream out(argv[2]);
    const std::string bad = ldpc::layer_partition_error(n, m, cp.data(), vi.data(), L, lp.data());
    if (!bad.empty()) {
        out << "partition_error " << bad << '\n';
        return 0;
    }
    const ldpc::LayerPlan p = ldpc::layer_plan(n, m, cp.data(), vi.data(), L, lp.data(), kind);
    put(out, "ok", std::vector<int>{p.ok ? 1 : 0});
    if (!p.ok) {
        out << "why " << p.why << '\n';
        return 0;
    }
    put(out, "scalars", std::vector<long long>{p.n, p.m, p.L, p.kind, p.W, p.G, p.lpc, p.threads, p.max_layer, p.entries,
                                               (long long)p.row_words, (long long)p.rec_off, (long long)p.lds_bytes,
                                               (long long)ldpc::layer_flag_words(p.G), (long long)ldpc::kLdsBytes,
                                               ldpc::kBlkMaxThreads, ldpc::kBlkMaxDeg});
    put(out, "layer_ptr", p.layer_ptr);
    put(out, "entry_base", p.entry_base);
    put(out, "deg", p.deg);
    put(out, "off", p.off);
    put(out, "edge_of_entry", p.edge_of_entry);
    return 0;
}
