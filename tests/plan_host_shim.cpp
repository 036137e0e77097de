// plan_host_shim.cpp -- the resident-plan builder (csrc/ldpc_plan.h) as a stand-alone host program, for
// tests/test_plan_host.py: built with g++ and the address / undefined-behaviour sanitizers, it never opens a GPU.
//
//   plan_host_shim IN OUT
// IN  (whitespace-separated integers): n m E, check_ptr[m+1], var_idx[E], then the planner inputs
//     dtype form T n_beta n_alpha n_oms_alpha beta_per_check rcq_zero0 has_oms_alpha, beta_slot[E], alpha_slot[n] and,
//     when has_oms_alpha, oms_alpha_slot[E].  The graph must be a valid CSR (the engine validates before it plans).
// OUT one line per item, "name count v0 v1 ...": the choice, every table of the general plan (res.*) and of the compact
//     plan (resc.*) that the engine would upload, and the compact grid and placement (cpt.*) whenever the graph has one --
//     the decoder's if it got a compact plan, else the one ldpc_debug_compact_* plan for a bare graph.
#include <cstdio>
#include <fstream>
#include <string>

#include "ldpc_plan.h"

using namespace ldpc;

namespace {

std::ofstream out;

template <typename It>
void put(const std::string &name, It first, It last)
{
    out << name << ' ' << (last - first);
    for (; first != last; ++first) out << ' ' << (long long)*first;
    out << '\n';
}
template <typename X>
void put(const std::string &name, const std::vector<X> &v) { put(name, v.begin(), v.end()); }
void put(const std::string &name, std::initializer_list<long long> v) { put(name, v.begin(), v.end()); }

void put(const std::string &name, const std::vector<Word2> &v)
{
    std::vector<uint32_t> flat;
    for (const Word2 &w : v) { flat.push_back(w.x); flat.push_back(w.y); }
    put(name, flat);
}

void put_tables(const std::string &p, const PlanTables &t)
{
    put(p + "scalars", {t.n, t.m, t.S, t.max_dc, t.max_dv, t.mstride, t.E, t.any_split, t.par_words, t.par_shift, t.n_hi,
                        t.n_pos, t.per_check, t.has_oaslot});
    put(p + "vcell", t.vcell, t.vcell + 8);
    put(p + "ccell", t.ccell, t.ccell + 8);
    put(p + "dc_s", t.dc_s);
    if (t.any_split) put(p + "gsz", t.gsz);
    put(p + "cvar", t.cvar);
    put(p + "bslot", t.bslot);
    if (t.per_check) put(p + "bslot_c", t.bslot_c);
    if (t.has_oaslot) put(p + "oaslot", t.oaslot);
    put(p + "vmeta", t.vmeta);
    put(p + "vslot_lo", t.vslot_lo);
    put(p + "vslot_hi", t.vslot_hi);
    put(p + "inv_perm_v", t.inv_perm_v);
    put(p + "edge_of_slot", t.edge_of_slot);
}

std::vector<int32_t> take(std::ifstream &in, long long count)
{
    std::vector<int32_t> v((size_t)count);
    for (int32_t &x : v) in >> x;
    return v;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    std::ifstream in(argv[1]);
    int n = 0, m = 0, E = 0;
    in >> n >> m >> E;
    const std::vector<int32_t> check_ptr = take(in, m + 1), var_idx = take(in, E);
    PlanInputs pi;
    int bpc = 0, z0 = 0, oms = 0;
    in >> pi.dtype >> pi.form >> pi.T >> pi.n_beta >> pi.n_alpha >> pi.n_oms_alpha >> bpc >> z0 >> oms;
    pi.beta_per_check = bpc; pi.rcq_zero0 = z0; pi.has_oms_alpha = oms;
    const std::vector<int32_t> beta_slot = take(in, E), alpha_slot = take(in, n), oms_slot = take(in, oms ? E : 0);
    if (!in) { std::fprintf(stderr, "short or malformed input\n"); return 2; }
    pi.beta_slot = beta_slot.data(); pi.alpha_slot = alpha_slot.data(); pi.oms_alpha_slot = oms ? oms_slot.data() : nullptr;

    HostGraph g;
    host_graph_fill(&g, n, m, E, check_ptr.data(), var_idx.data());
    out.open(argv[2]);
    put("graph", {g.n, g.m, g.E, g.max_dc, g.max_dv});

    ResidentChoice c = choose_resident_plan(&g, pi);
    put("choice", {c.res_ok, c.resc_ok, c.G, c.NT, (long long)c.res_lds, (long long)c.resc_lds});
    if (c.res_ok) put_tables("res.", c.res);
    if (c.resc_ok) put_tables("resc.", c.resc);

    std::vector<ResVCheck> vc;
    long long Sc = 0;
    if (resident_checks(&g, vc) && cpt_geometry(&g, vc, Sc)) {
        if (!c.resc_ok) cpt_layout(&g, vc, Sc, c.resc_layout);
        const CptLayout &L = c.resc_layout;
        unsigned words[kCptWaves];
        cpt_check_words(vc, true, words);
        std::vector<int> check_of_pos, base_check_of_pos;
        for (int k : L.check_at) check_of_pos.push_back(vc[k].check);
        for (int k : L.base_check_at) base_check_of_pos.push_back(vc[k].check);
        put("cpt.geometry", {kResCptStride, Sc});
        put("cpt.var_at", L.var_at);
        put("cpt.cell", L.cell, L.cell + kCptWaves);
        put("cpt.stats", {(long long)L.var_at.size(), L.worst, L.total, L.mixed});
        put("cpt.words", words, words + kCptWaves);
        put("cpt.slot_of_edge", L.slot_of_edge);
        put("cpt.check_of_pos", check_of_pos);
        put("cpt.banks", L.banks, L.banks + 4);
        put("cpt.base_slot_of_edge", L.base_slot_of_edge);
        put("cpt.base_check_of_pos", base_check_of_pos);
        put("cpt.base_banks", L.base_banks, L.base_banks + 4);
    }
    out.close();
    return out ? 0 : 1;
}
