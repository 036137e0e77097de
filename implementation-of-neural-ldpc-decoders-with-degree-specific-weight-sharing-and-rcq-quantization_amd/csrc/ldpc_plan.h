// ldpc_plan.h -- host planner of the LDS-resident engine (kernels: ldpc_resident.hip).
//
// Pure integer C++17 on host vectors: which geometry a code gets (choose_resident_plan), the slot layout and per-slot
// tables of one geometry (resident_layout) and the compact plan's grid and bank-aware placement (cpt_*).  Nothing here
// knows a device: the tables come back as host data, the engine uploads them, and a host test drives the planner in a
// process of its own.
#pragma once

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "ldpc_resident_geom.h"

namespace ldpc {

// host copies of a graph: CSR as given, CSC with every variable's edges in ascending check order
struct HostGraph {
    int n = 0, m = 0, E = 0, max_dc = 0, max_dv = 0;
    std::vector<int> h_check_ptr, h_var_idx, h_var_ptr, h_csc, h_check_of_edge;
};

// fills g from a VALID CSR (sizes consistent, var_idx in range): CSC by scanning the CSR edges in order
inline void host_graph_fill(HostGraph *g, int n, int m, int E, const int32_t *check_ptr, const int32_t *var_idx)
{
    g->n = n; g->m = m; g->E = E; g->max_dc = g->max_dv = 0;
    g->h_check_ptr.assign(check_ptr, check_ptr + m + 1);
    g->h_var_idx.assign(var_idx, var_idx + E);
    g->h_var_ptr.assign((size_t)n + 1, 0);
    g->h_check_of_edge.resize(E);
    for (int i = 0; i < m; ++i) {
        g->max_dc = std::max(g->max_dc, check_ptr[i + 1] - check_ptr[i]);
        for (int e = check_ptr[i]; e < check_ptr[i + 1]; ++e) { g->h_check_of_edge[e] = i; g->h_var_ptr[var_idx[e] + 1]++; }
    }
    for (int j = 0; j < n; ++j) {
        g->max_dv = std::max(g->max_dv, g->h_var_ptr[j + 1]);
        g->h_var_ptr[j + 1] += g->h_var_ptr[j];
    }
    std::vector<int> fill(g->h_var_ptr.begin(), g->h_var_ptr.end() - 1);
    g->h_csc.resize(E);
    for (int e = 0; e < E; ++e) g->h_csc[fill[var_idx[e]]++] = e;
}

// what the planner reads of a decoder and its description.  dtype and form carry the values of the C ABI's LDPC_F32 /
// LDPC_F64 and LDPC_C2V_* (the engine asserts the equality)
enum { kPlanF32 = 0, kPlanF64 = 1 };
enum { kPlanNMS = 0, kPlanRCQ = 1, kPlanOMS = 2 };
struct PlanInputs {
    int dtype = kPlanF32, form = kPlanNMS, T = 0;
    int n_beta = 0, n_alpha = 0, n_oms_alpha = 0;
    bool beta_per_check = false;                  // every edge of a check uses the same beta slot
    bool rcq_zero0 = false;                       // every quantiser's tau_0 == 0
    bool has_oms_alpha = false;                   // an OMS alpha table exists (oms_alpha_slot is read)
    const int32_t *beta_slot = nullptr, *alpha_slot = nullptr, *oms_alpha_slot = nullptr;   // [E], [n], [E]
};

struct Word2 { uint32_t x, y; };                  // two words of a packed table (the device's uint2)


// Compact plan: variables on a (round, wave, lane) grid.
// The compact kernel (kResCptThreads = 512 lanes, kResRegVars = 4 rounds) runs the variable at position
// q = r*512 + w*64 + lane in round r of wave w.  Every variable phase ends at a workgroup barrier, so the phase costs
// what its busiest wave costs; a cell (w, r) whose 64 lanes share one degree runs one body behind a scalar branch
// (ResidentPlan::vcell), a mixed cell runs the body of every degree it holds.  Cost of one body, in VALU-equivalents,
// from the instruction model (not from ISA counts): dv leave-one-out sums of dv-1 terms each, formed separately in the
// reference's association order (<= dv*(dv-1) adds), 2*dv LDS operations and ~4 for the offset unpacking.
constexpr int kCptWaves = kResCptThreads / 64;
constexpr int kCptCells = kCptWaves * kResRegVars;
constexpr int kCptMaxDv = 8;
constexpr long kCptJointTrials = 3000000;    // budget of the joint bank-aware placement search (cpt_place_banks)
inline int cpt_body_cost(int dv) { return dv * (dv - 1) + 2 * dv + 4; }

struct CptLayout {
    std::vector<int> var_at;       // [n_pos] variable at grid position q, -1 = empty
    unsigned cell[kCptWaves] = {}; // ResidentPlan::vcell
    int worst = 0, total = 0;      // largest and summed per-wave cost of one variable phase (cpt_body_cost model)
    int mixed = 0;                 // cells of kind kCellMixed
    // slot placement (cpt_place_banks): check position p runs the check vc[check_at[p]] of the degree-sorted list, edge e
    // sits in slot slot_of_edge[e] = row * kResCptStride + p.  banks = { gather cost, gather groups, scatter cost,
    // scatter groups } of one variable phase under the LDS model (BankModel); base_* is the same for the placement of
    // the stable check order with rows in CSR order and the variables-only search, the starting point of the joint one
    std::vector<int> check_at, slot_of_edge, base_check_at, base_slot_of_edge;
    int banks[4] = {}, base_banks[4] = {};
};

// a lane position of the check phase: (sub-)check `check`, its edges e0 .. e0+dc-1, lane-group size gs
struct ResVCheck { int check, e0, dc, gs; };

inline int resident_alpha_floats(int dtype, int T, int n_alpha)
{
    if (dtype != kPlanF32) return 0;                    // the fp64 kernel reads alpha from global memory
    const long long cnt = (long long)T * n_alpha;
    return cnt <= kResAlphaMax ? (int)cnt : 0;
}

// G codewords per workgroup fit when the state is within LDS and slot byte offsets fit 16 bits
inline bool resident_fits(const PlanInputs &in, int n, long long S, int G, int blocks, int m_par)
{
    if (S * G * 4 > 65535) return false;
    return blocks * res_lds_total((int)S, n, G, resident_alpha_floats(in.dtype, in.T, in.n_alpha), m_par) <= kLdsBytes;
}
inline bool is_pow2(int x) { return x > 0 && (x & (x - 1)) == 0; }

// ---- LDS bank-conflict-aware lane assignment -------------------------------------------------
// The check phase touches consecutive slots (conflict-free by construction); the variable phase
// gathers/scatters the slots of a variable's edges, so which variables share a wave decides how
// many LDS passes those accesses take.  Any order of the variables INSIDE a degree class is valid,
// so a seeded hill climb swaps variables between lane groups whenever that lowers
//     sum over read groups  (32 lanes) of  max multiplicity of (slot mod RM)
//   + sum over write groups (WG lanes) of  max multiplicity of (slot mod WM)
// (RM/WG/WM follow the instruction's banking: ds_read_b64 64 banks, ds_write_b64 32 banks in
// 16-lane groups; MI355X_MICROARCH.md "LDS").  On the (1998,1512) code the gathers go from 3.3 to
// ~2.1 passes per instruction, the scatters from 2.9 to ~2.0.  Purely a performance choice.
struct LaneCost {
    const std::vector<std::vector<int>> &vs;   // slots of each variable, CSC order
    const std::vector<int> &order;
    int rg, rm, wg, wm;
    int group(int first, int count, int mod) const
    {
        const int last = std::min<int>(first + count, (int)order.size());
        int kmax = 0;
        for (int i = first; i < last; ++i) kmax = std::max<int>(kmax, (int)vs[order[i]].size());
        int cost = 0;
        unsigned char cnt[64];
        for (int k = 0; k < kmax; ++k) {
            std::memset(cnt, 0, sizeof(cnt));
            int mx = 0;
            for (int i = first; i < last; ++i) {
                const auto &v = vs[order[i]];
                if ((int)v.size() > k) mx = std::max<int>(mx, ++cnt[v[k] % mod]);
            }
            cost += mx;
        }
        return cost;
    }
    int around(int x, int y) const            // cost of every group containing position x or y
    {
        int c = group(x / rg * rg, rg, rm) + group(x / wg * wg, wg, wm);
        if (y / rg != x / rg) c += group(y / rg * rg, rg, rm);
        if (y / wg != x / wg) c += group(y / wg * wg, wg, wm);
        return c;
    }
};

inline void optimise_lane_order(std::vector<int> &order, const std::vector<std::vector<int>> &vs, int G)
{
    if (G != 1 && G != 2) return;
    LaneCost lc{vs, order, 32, 32, G == 2 ? 16 : 32, G == 2 ? 16 : 32};
    const int n = (int)order.size();
    std::vector<std::pair<int, int>> classes;
    for (int i = 0; i < n;) {
        int j = i;
        while (j < n && vs[order[j]].size() == vs[order[i]].size()) ++j;
        if (j - i >= 2 && !vs[order[i]].empty()) classes.push_back({i, j});
        i = j;
    }
    if (classes.empty()) return;
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    const long trials = std::min<long>(400000, 150L * n);
    for (long it = 0; it < trials; ++it) {
        const auto &c = classes[next() % classes.size()];
        const int x = c.first + (int)(next() % (uint64_t)(c.second - c.first));
        const int y = c.first + (int)(next() % (uint64_t)(c.second - c.first));
        if (x / lc.wg == y / lc.wg) continue;
        const int before = lc.around(x, y);
        std::swap(order[x], order[y]);
        if (lc.around(x, y) > before) std::swap(order[x], order[y]);
    }
}

// Lane positions of the check phase are VIRTUAL checks.  A check of degree <= kResSubDegreeCap is one of them; a wider
// one is split into 2^k sub-checks of contiguous edges (balanced, at most kResSubDegree each) that sit on ADJACENT lanes
// and are combined by wavefront exchanges (ldpc_resident.hip: group_combine).  Groups come first, by descending size --
// every group then starts at a multiple of its size, so it never straddles a wave -- then the whole checks.
inline bool resident_checks(const HostGraph *g, std::vector<ResVCheck> &vc)
{
    auto dc_real = [&](int i) { return g->h_check_ptr[i + 1] - g->h_check_ptr[i]; };
    std::vector<int> wide_ids, plain_ids;
    for (int i = 0; i < g->m; ++i) (dc_real(i) > kResSubDegreeCap ? wide_ids : plain_ids).push_back(i);
    auto group_of = [&](int i) { int k = 1; while (k * kResSubDegree < dc_real(i)) k <<= 1; return k; };
    for (int i : wide_ids)
        if (group_of(i) > 64) return false;                 // wider than a wavefront of sub-checks
    std::stable_sort(wide_ids.begin(), wide_ids.end(), [&](int a, int b) { return group_of(a) > group_of(b); });
    for (int i : wide_ids) {
        const int k = group_of(i), dc = dc_real(i), base = dc / k, rem = dc % k;
        int e = g->h_check_ptr[i];
        for (int j = 0; j < k; ++j) {
            const int len = base + (j < rem ? 1 : 0);
            vc.push_back({i, e, len, k});
            e += len;
        }
    }
    std::stable_sort(plain_ids.begin(), plain_ids.end(), [&](int a, int b) { return dc_real(a) > dc_real(b); });
    for (int i : plain_ids) vc.push_back({i, g->h_check_ptr[i], dc_real(i), 1});
    return true;
}

// ---- compact plan: variables on a (round, wave, lane) grid (CptLayout) --------------------------
// cell bytes and model costs of a grid (any placement: the balanced one or the degree-sorted fallback)
inline void cpt_cells(const std::vector<int> &dv, CptLayout &L)
{
    const int n_pos = (int)L.var_at.size();
    L.worst = L.total = L.mixed = 0;
    for (int w = 0; w < kCptWaves; ++w) {
        L.cell[w] = 0;
        int wave = 0;
        for (int r = 0; r < kResRegVars; ++r) {
            bool has[kCptMaxDv + 1] = {};
            int used = 0, kinds = 0, deg = 0, cost = 0;
            for (int lane = 0; lane < 64; ++lane) {
                const int q = r * kResCptThreads + w * 64 + lane;
                const int j = q < n_pos ? L.var_at[q] : -1;
                if (j < 0) continue;
                ++used;
                if (!has[dv[j]]) { has[dv[j]] = true; ++kinds; deg = dv[j]; cost += cpt_body_cost(dv[j]); }
            }
            unsigned byte = kCellEmpty;
            if (used) byte = (kinds == 1 && deg > 0) ? (unsigned)deg | (used < 64 ? kCellHoles : 0u) : kCellMixed;
            L.mixed += byte == kCellMixed ? 1 : 0;
            L.cell[w] |= byte << (8 * r);
            wave += cost;
        }
        L.worst = std::max(L.worst, wave);
        L.total += wave;
    }
}

// Balanced placement.  Cells are formed per degree (full cells of 64, one partial cell per degree); partial cells are
// merged -- the pair whose merged cell costs least -- or, when no pair fits 64 lanes, the smallest one is poured into
// the others' free lanes, until there are at most kCptCells cells and at most kCptWaves of them hold a degree > 4
// (those need the upper offset half, which only round 0 carries).  Degree > 4 cells go to round 0 of distinct waves,
// the others largest first to the cheapest wave with a free round; pairwise moves then lower the largest wave cost,
// and the waves are ordered so that w and w + 4 (assumed to share a SIMD) carry equal totals.  Deterministic.
inline bool cpt_assign(const std::vector<int> &dv, CptLayout &L)
{
    struct Cell { int cnt[kCptMaxDv + 1] = {}; int size = 0; };
    auto hi = [](const Cell &c) { for (int d = 5; d <= kCptMaxDv; ++d) if (c.cnt[d]) return true; return false; };
    auto cost = [](const Cell &c) { int k = 0; for (int d = 0; d <= kCptMaxDv; ++d) if (c.cnt[d]) k += cpt_body_cost(d); return k; };
    const int n = (int)dv.size();
    int cnt[kCptMaxDv + 1] = {};
    for (int j = 0; j < n; ++j) {
        if (dv[j] < 0 || dv[j] > kCptMaxDv) return false;
        ++cnt[dv[j]];
    }
    std::vector<Cell> cells;
    std::vector<char> partial;
    for (int d = kCptMaxDv; d >= 0; --d) {
        for (int k = cnt[d]; k > 0; k -= 64) {
            Cell c; c.cnt[d] = c.size = std::min(k, 64);
            cells.push_back(c);
            partial.push_back(c.size < 64);
        }
    }
    for (;;) {
        int nhi = 0;
        for (const Cell &c : cells) nhi += hi(c) ? 1 : 0;
        const bool need_hi = nhi > kCptWaves;
        if (!need_hi && (int)cells.size() <= kCptCells) break;
        int a = -1, b = -1, best = INT_MAX;
        for (int i = 0; i < (int)cells.size(); ++i)
            for (int k = i + 1; k < (int)cells.size(); ++k) {
                if (cells[i].size + cells[k].size > 64 || (need_hi && !(hi(cells[i]) && hi(cells[k])))) continue;
                Cell m = cells[i];
                for (int d = 0; d <= kCptMaxDv; ++d) m.cnt[d] += cells[k].cnt[d];
                if (cost(m) < best) { best = cost(m); a = i; b = k; }
            }
        if (a < 0) {                                     // pour the smallest suitable cell into the others' free lanes
            int src = -1;
            for (int pass = 0; pass < 2 && src < 0; ++pass)
                for (int i = 0; i < (int)cells.size(); ++i) {
                    if (cells[i].size == 64 || hi(cells[i]) != (need_hi || pass == 1)) continue;
                    if (src < 0 || cells[i].size < cells[src].size) src = i;
                }
            if (src < 0) return false;
            const bool src_hi = hi(cells[src]);
            for (int d = kCptMaxDv; d >= 0; --d)
                while (cells[src].cnt[d] > 0) {
                    int t = -1;
                    for (int i = 0; i < (int)cells.size(); ++i) {
                        if (i == src || cells[i].size == 64 || (src_hi && !hi(cells[i]))) continue;
                        if (t < 0 || cells[i].size < cells[t].size) t = i;
                    }
                    if (t < 0) return false;
                    const int k = std::min(cells[src].cnt[d], 64 - cells[t].size);
                    cells[t].cnt[d] += k; cells[t].size += k;
                    cells[src].cnt[d] -= k; cells[src].size -= k;
                }
            cells.erase(cells.begin() + src);
            continue;
        }
        for (int d = 0; d <= kCptMaxDv; ++d) cells[a].cnt[d] += cells[b].cnt[d];
        cells[a].size += cells[b].size;
        cells.erase(cells.begin() + b);
    }

    // placement: slot[w][r] = cell index or -1
    int slot[kCptWaves][kResRegVars];
    for (auto &w : slot) for (int &x : w) x = -1;
    int load[kCptWaves] = {};
    std::vector<int> order((size_t)cells.size());
    for (int i = 0; i < (int)cells.size(); ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
        if (hi(cells[x]) != hi(cells[y])) return hi(cells[x]);
        return cost(cells[x]) > cost(cells[y]);
    });
    int next_hi = 0;
    for (int i : order) {
        if (hi(cells[i])) { slot[next_hi][0] = i; load[next_hi++] += cost(cells[i]); continue; }
        int bw = -1;
        for (int w = 0; w < kCptWaves; ++w) {
            bool free_ = false;
            for (int r = 0; r < kResRegVars; ++r) free_ = free_ || slot[w][r] < 0;
            if (free_ && (bw < 0 || load[w] < load[bw])) bw = w;
        }
        if (bw < 0) return false;
        for (int r = 0; r < kResRegVars; ++r)
            if (slot[bw][r] < 0) { slot[bw][r] = i; break; }
        load[bw] += cost(cells[i]);
    }
    // pairwise exchanges (a cell with an empty slot included): largest wave cost first, then the sum of squares
    auto objective = [&](long long &mx, long long &sq) {
        mx = 0; sq = 0;
        for (int w = 0; w < kCptWaves; ++w) { mx = std::max<long long>(mx, load[w]); sq += (long long)load[w] * load[w]; }
    };
    for (bool improved = true; improved;) {
        improved = false;
        for (int x = 0; x < kCptCells; ++x)
            for (int y = x + 1; y < kCptCells; ++y) {
                const int wx = x / kResRegVars, rx = x % kResRegVars, wy = y / kResRegVars, ry = y % kResRegVars;
                const int cx = slot[wx][rx], cy = slot[wy][ry];
                if (wx == wy || (cx < 0 && cy < 0)) continue;
                if ((cx >= 0 && hi(cells[cx]) && ry != 0) || (cy >= 0 && hi(cells[cy]) && rx != 0)) continue;
                long long m0, s0, m1, s1;
                objective(m0, s0);
                const int kx = cx >= 0 ? cost(cells[cx]) : 0, ky = cy >= 0 ? cost(cells[cy]) : 0;
                load[wx] += ky - kx; load[wy] += kx - ky;
                objective(m1, s1);
                if (m1 < m0 || (m1 == m0 && s1 < s0)) { std::swap(slot[wx][rx], slot[wy][ry]); improved = true; }
                else { load[wx] -= ky - kx; load[wy] -= kx - ky; }
            }
    }
    // waves w and w + 4: the heaviest with the lightest, and so on
    int by_load[kCptWaves];
    for (int w = 0; w < kCptWaves; ++w) by_load[w] = w;
    std::stable_sort(by_load, by_load + kCptWaves, [&](int x, int y) { return load[x] > load[y]; });
    int wave_of[kCptWaves];                              // new wave index -> old one
    for (int k = 0; k < kCptWaves / 2; ++k) {
        wave_of[k] = by_load[k];
        wave_of[k + kCptWaves / 2] = by_load[kCptWaves - 1 - k];
    }
    // inside a wave: the degree > 4 cell in round 0, then by falling cost, empty rounds last
    std::vector<std::vector<int>> of_deg(kCptMaxDv + 1);
    for (int j = 0; j < n; ++j) of_deg[dv[j]].push_back(j);
    size_t taken[kCptMaxDv + 1] = {};
    L.var_at.assign((size_t)kCptCells * 64, -1);
    for (int w = 0; w < kCptWaves; ++w) {
        int cs[kResRegVars];
        for (int r = 0; r < kResRegVars; ++r) cs[r] = slot[wave_of[w]][r];
        std::stable_sort(cs, cs + kResRegVars, [&](int x, int y) {
            if (x < 0 || y < 0) return x >= 0 && y < 0;
            if (hi(cells[x]) != hi(cells[y])) return hi(cells[x]);
            return cost(cells[x]) > cost(cells[y]);
        });
        for (int r = 0; r < kResRegVars; ++r) {
            if (cs[r] < 0) continue;
            int lane = 0;
            for (int d = kCptMaxDv; d >= 0; --d)
                for (int k = 0; k < cells[cs[r]].cnt[d]; ++k)
                    L.var_at[(size_t)r * kResCptThreads + w * 64 + lane++] = of_deg[d][taken[d]++];
        }
    }
    int n_pos = 0;
    for (int q = 0; q < (int)L.var_at.size(); ++q)
        if (L.var_at[q] >= 0) n_pos = q + 1;
    L.var_at.resize((size_t)n_pos);
    cpt_cells(dv, L);
    return true;
}

// ---- compact plan: joint bank-aware slot placement ------------------------------------------------
// The LDS model of one variable phase of the compact kernels (codeword pairs: 8-byte slots).  The lane at grid position q
// gathers and scatters the slot of its variable's k-th edge (CSC order) with the k-th ds_read_b64 / ds_write_b64 of its
// round; a read resolves 32 lanes per LDS cycle on slot mod 32, a write 16 lanes on slot mod 16, and a group takes as
// many cycles as its fullest bank holds lanes.  Three things are free and change no result: which variables of one
// degree share a lane group, which position a check takes among the checks of its degree (the per-wave degrees, so
// ccell and Sc, stay), and which row each edge of a check takes (min1, min2 and the sign parity do not depend on the
// order of the edges; every per-slot table is filled from the same map).  BankModel keeps one bank histogram per
// (group, k) and evaluates a move from the entries it changes; every move is its own inverse.
struct BankModel {
    static constexpr int kRG = 32, kRM = 32, kWG = 16, kWM = 16;
    const HostGraph *g;
    const std::vector<ResVCheck> &vc;
    std::vector<int> &var_at, &check_at, &slot_of_edge;
    std::vector<int> pos_of_var, k_of_edge, edge_at;     // edge_at[vc[c].e0 + t] = the edge in row t of check c
    std::vector<unsigned char> hist[2], mx[2];           // [0] gathers, [1] scatters: [cell][bank], [cell]
    std::vector<int> dirty;                              // cells whose fullest bank lost a lane: kind | cell << 1
    long long cost = 0, sq = 0;                          // sum of the cells' maxima; sum of the squared bank counts

    BankModel(const HostGraph *g_, const std::vector<ResVCheck> &vc_, std::vector<int> &var_at_,
              std::vector<int> &check_at_, std::vector<int> &slot_of_edge_)
        : g(g_), vc(vc_), var_at(var_at_), check_at(check_at_), slot_of_edge(slot_of_edge_)
    {
        const int n_pos = (int)var_at.size();
        pos_of_var.assign(g->n, -1);
        for (int q = 0; q < n_pos; ++q)
            if (var_at[q] >= 0) pos_of_var[var_at[q]] = q;
        k_of_edge.assign(g->E, 0);
        for (int j = 0; j < g->n; ++j)
            for (int s = g->h_var_ptr[j]; s < g->h_var_ptr[j + 1]; ++s) k_of_edge[g->h_csc[s]] = s - g->h_var_ptr[j];
        edge_at.assign(g->E, 0);
        for (const ResVCheck &v : vc)
            for (int t = 0; t < v.dc; ++t) edge_at[v.e0 + t] = v.e0 + t;
        const int rcells = (n_pos + kRG - 1) / kRG * kCptMaxDv, wcells = (n_pos + kWG - 1) / kWG * kCptMaxDv;
        hist[0].assign((size_t)rcells * kRM, 0); mx[0].assign(rcells, 0);
        hist[1].assign((size_t)wcells * kWM, 0); mx[1].assign(wcells, 0);
        for (int e = 0; e < g->E; ++e) entry(e, +1);
        settle();
    }
    void bump(int kind, int cell, int banks, int bank, int sign)
    {
        unsigned char &c = hist[kind][(size_t)cell * banks + bank];
        if (sign > 0) {
            sq += 2 * c + 1;
            if (++c > mx[kind][cell]) { mx[kind][cell] = c; ++cost; }
        } else {
            sq -= 2 * c - 1;
            if (c-- == mx[kind][cell]) dirty.push_back(kind | cell << 1);
        }
    }
    void entry(int e, int sign)                          // edge e's accesses enter (+1) or leave (-1) the histograms
    {
        const int q = pos_of_var[g->h_var_idx[e]], k = k_of_edge[e], s = slot_of_edge[e];
        bump(0, q / kRG * kCptMaxDv + k, kRM, s % kRM, sign);
        bump(1, q / kWG * kCptMaxDv + k, kWM, s % kWM, sign);
    }
    void settle()                                        // exact maxima of the dirty cells
    {
        for (int dc : dirty) {
            const int kind = dc & 1, cell = dc >> 1, banks = kind ? kWM : kRM;
            const unsigned char *h = &hist[kind][(size_t)cell * banks];
            unsigned char m = 0;
            for (int b = 0; b < banks; ++b) m = std::max(m, h[b]);
            cost += (int)m - (int)mx[kind][cell];
            mx[kind][cell] = m;
        }
        dirty.clear();
    }
    void swap_vars(int x, int y)                         // grid positions of two variables
    {
        const int jx = var_at[x], jy = var_at[y];
        for (int j : {jx, jy})
            for (int s = g->h_var_ptr[j]; s < g->h_var_ptr[j + 1]; ++s) entry(g->h_csc[s], -1);
        std::swap(var_at[x], var_at[y]);
        pos_of_var[jx] = y; pos_of_var[jy] = x;
        for (int j : {jx, jy})
            for (int s = g->h_var_ptr[j]; s < g->h_var_ptr[j + 1]; ++s) entry(g->h_csc[s], +1);
        settle();
    }
    void swap_checks(int p, int r)                       // two positions that hold checks of one degree
    {
        const ResVCheck &a = vc[check_at[p]], &b = vc[check_at[r]];
        for (int t = 0; t < a.dc; ++t) { entry(a.e0 + t, -1); entry(b.e0 + t, -1); }
        for (int t = 0; t < a.dc; ++t) { slot_of_edge[a.e0 + t] += r - p; slot_of_edge[b.e0 + t] += p - r; }
        for (int t = 0; t < a.dc; ++t) { entry(a.e0 + t, +1); entry(b.e0 + t, +1); }
        std::swap(check_at[p], check_at[r]);
        settle();
    }
    void swap_rows(int p, int t, int u)                  // two rows of the check at position p
    {
        const ResVCheck &a = vc[check_at[p]];
        const int e = edge_at[a.e0 + t], f = edge_at[a.e0 + u];
        entry(e, -1); entry(f, -1);
        std::swap(slot_of_edge[e], slot_of_edge[f]);
        std::swap(edge_at[a.e0 + t], edge_at[a.e0 + u]);
        entry(e, +1); entry(f, +1);
        settle();
    }
    void report(int (&out)[4]) const                     // { gather cost, gather groups, scatter cost, scatter groups }
    {
        for (int kind = 0; kind < 2; ++kind) {
            int c = 0, groups = 0;
            for (unsigned char m : mx[kind]) { c += m; groups += m ? 1 : 0; }
            out[2 * kind] = c; out[2 * kind + 1] = groups;
        }
    }
};

// Seeded local search over L.var_at, L.check_at and L.slot_of_edge, budgeted by trial counts alone (deterministic).
// First the variables-only climb on the summed maxima that this planner has always run (same moves, same acceptance, same
// random sequence); its result is recorded as the baseline.  Then the joint climb: swaps of two variables of one degree,
// of two checks of one degree, of two rows of one check, accepted when the summed maxima fall, or stay while the summed
// squared bank counts do not rise -- the second term keeps a gradient once every group sits at two lanes per bank.
inline void cpt_place_banks(const HostGraph *g, const std::vector<ResVCheck> &vc, CptLayout &L)
{
    const int n = g->n, m = (int)vc.size();
    L.check_at.resize(m);
    L.slot_of_edge.assign(g->E, 0);
    for (int p = 0; p < m; ++p) {
        L.check_at[p] = p;
        for (int t = 0; t < vc[p].dc; ++t) L.slot_of_edge[vc[p].e0 + t] = t * kResCptStride + p;
    }
    BankModel bm(g, vc, L.var_at, L.check_at, L.slot_of_edge);
    std::vector<std::vector<int>> vclass(kCptMaxDv + 1);                // grid positions by variable degree
    for (int q = 0; q < (int)L.var_at.size(); ++q) {
        if (L.var_at[q] < 0) continue;
        const int d = g->h_var_ptr[L.var_at[q] + 1] - g->h_var_ptr[L.var_at[q]];
        if (d > 0 && d <= kCptMaxDv) vclass[d].push_back(q);
    }
    vclass.erase(std::remove_if(vclass.begin(), vclass.end(), [](const std::vector<int> &c) { return c.size() < 2; }),
                 vclass.end());
    std::vector<std::pair<int, int>> cclass;                            // [first, last) positions of one check degree
    std::vector<int> rowable;                                           // positions whose check has two rows or more
    for (int p = 0; p < m;) {
        int r = p;
        while (r < m && vc[r].dc == vc[p].dc) ++r;
        if (r - p >= 2 && vc[p].dc > 0) cclass.push_back({p, r});
        p = r;
    }
    for (int p = 0; p < m; ++p)
        if (vc[p].dc >= 2) rowable.push_back(p);
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    if (!vclass.empty()) {
        const long trials = std::min<long>(400000, 150L * n);
        for (long it = 0; it < trials; ++it) {
            const auto &c = vclass[next() % vclass.size()];
            const int x = c[next() % c.size()], y = c[next() % c.size()];
            if (x / BankModel::kWG == y / BankModel::kWG) continue;
            const long long before = bm.cost;
            bm.swap_vars(x, y);
            if (bm.cost > before) bm.swap_vars(x, y);
        }
    }
    bm.report(L.base_banks);
    L.base_check_at = L.check_at;
    L.base_slot_of_edge = L.slot_of_edge;

    // rows are the cheapest move and the most productive: 29 trials in 32; 2 move variables, 1 moves checks
    const long joint = std::min<long>(kCptJointTrials, 500L * g->E);
    for (long it = 0; it < joint; ++it) {
        const long long cost0 = bm.cost, sq0 = bm.sq;
        const unsigned kind = (unsigned)(next() % 32);
        int a = 0, b = 0, c = 0;
        if (kind < 2) {
            if (vclass.empty()) continue;
            const auto &cl = vclass[next() % vclass.size()];
            a = cl[next() % cl.size()]; b = cl[next() % cl.size()];
            if (a / BankModel::kWG == b / BankModel::kWG) continue;
            bm.swap_vars(a, b);
        } else if (kind < 3) {
            if (cclass.empty()) continue;
            const auto &cl = cclass[next() % cclass.size()];
            a = cl.first + (int)(next() % (uint64_t)(cl.second - cl.first));
            b = cl.first + (int)(next() % (uint64_t)(cl.second - cl.first));
            if (a == b) continue;
            bm.swap_checks(a, b);
        } else {
            if (rowable.empty()) continue;
            a = rowable[next() % rowable.size()];
            const int dc = vc[L.check_at[a]].dc;
            b = (int)(next() % (uint64_t)dc); c = (int)(next() % (uint64_t)dc);
            if (b == c) continue;
            bm.swap_rows(a, b, c);
        }
        if (bm.cost < cost0 || (bm.cost == cost0 && bm.sq <= sq0)) continue;
        if (kind < 2) bm.swap_vars(a, b);
        else if (kind < 3) bm.swap_checks(a, b);
        else bm.swap_rows(a, b, c);
    }
    bm.report(L.banks);
}

// the compact geometry's slot count Sc when the graph qualifies: no split checks, m <= kResCptStride, the variables within
// kResRegVars rounds of 512 lanes with every degree > 4 one in round 0, 16-bit slot offsets, the LLR rows stageable in the
// slot area (cpt_layout keeps its positions below Sc) and kResCptBlocks workgroups per CU
inline bool cpt_geometry(const HostGraph *g, const std::vector<ResVCheck> &vc, long long &Sc)
{
    const int n = g->n, m = (int)vc.size();
    int max_sub = 0;
    for (const ResVCheck &v : vc) max_sub = std::max(max_sub, v.dc);
    if (m != g->m || m > kResCptStride || n > kResRegVars * kResCptThreads || g->max_dv > kCptMaxDv || max_sub < 1)
        return false;
    int n_top = 0;
    while (n_top < m && vc[n_top].dc == max_sub) ++n_top;
    Sc = (long long)(max_sub - 1) * kResCptStride + n_top;
    int n_hi = 0;
    for (int j = 0; j < n; ++j) n_hi += (g->h_var_ptr[j + 1] - g->h_var_ptr[j]) > 4 ? 1 : 0;
    return Sc * 2 * 4 <= 65535 && (long long)n <= Sc && n_hi <= kResCptThreads &&
           kResCptBlocks * res_cpt_lds_total((int)Sc, 2) <= kLdsBytes;
}

// the compact plan's check table (ResidentPlan::ccell): wave w holds the checks at positions 64w .. 64w+63.  `select_form`:
// the decoder's check phase is the one-beta-per-check select form, the only one with a scalar-counted body
inline void cpt_check_words(const std::vector<ResVCheck> &vc, bool select_form, unsigned (&words)[kCptWaves])
{
    const int m = (int)vc.size();
    for (int w = 0; w < kCptWaves; ++w) {
        const int p0 = std::min(64 * w, m), p1 = std::min(p0 + 64, m);
        int lo = p0 < p1 ? 255 : 0, hi = 0;
        for (int p = p0; p < p1; ++p) { lo = std::min(lo, vc[p].dc); hi = std::max(hi, vc[p].dc); }
        words[w] = p0 < p1 ? chk_word(lo, hi, p1 - p0) | (select_form ? 0u : kChkPerLane) : 0u;
    }
}

// the compact plan's grid for a graph and its check order: the balanced placement, else (a staging area too small for its
// positions) the degree-sorted order of the general plan; then variables, check positions and edge rows are placed for LDS
// banking (cpt_place_banks)
inline void cpt_layout(const HostGraph *g, const std::vector<ResVCheck> &vc, long long S, CptLayout &L)
{
    const int n = g->n;
    std::vector<int> dv(n);
    for (int j = 0; j < n; ++j) dv[j] = g->h_var_ptr[j + 1] - g->h_var_ptr[j];
    if (!cpt_assign(dv, L) || (long long)L.var_at.size() > S) {
        L.var_at.resize(n);
        for (int j = 0; j < n; ++j) L.var_at[j] = j;
        std::stable_sort(L.var_at.begin(), L.var_at.end(), [&](int a, int b) { return dv[a] > dv[b]; });
    }
    cpt_place_banks(g, vc, L);
    cpt_cells(dv, L);
}

// host image of one ResidentPlan (ldpc_resident.hip): its scalar fields and every table the engine uploads
struct PlanTables {
    int n = 0, m = 0, S = 0, max_dc = 0, max_dv = 0, mstride = 0, E = 0;
    int any_split = 0, par_words = 0, par_shift = 0, n_hi = 0, n_pos = 0;
    unsigned vcell[8] = {}, ccell[8] = {};
    bool per_check = false, has_oaslot = false;   // bslot_c / oaslot are part of the plan (gsz: any_split)
    std::vector<uint8_t> dc_s, gsz;
    std::vector<uint16_t> cvar, bslot, bslot_c, oaslot, inv_perm_v;
    std::vector<uint32_t> vmeta, edge_of_slot;
    std::vector<Word2> vslot_lo, vslot_hi;
};

// slot layout of one geometry: row stride `mstride`, S slots, G codewords per slot; variables ordered inside their degree
// classes for LDS banking (general plan) or at the positions of the compact grid `cl`
inline PlanTables resident_layout(const HostGraph *g, const PlanInputs &in, const std::vector<ResVCheck> &sorted, int mstride,
                                  long long S, int G, const CptLayout *cl = nullptr)
{
    std::vector<ResVCheck> placed;                               // compact plan: the checks in position order
    if (cl)
        for (int c : cl->check_at) placed.push_back(sorted[c]);
    const std::vector<ResVCheck> &vc = cl ? placed : sorted;
    const int n = g->n, m = (int)vc.size();
    const bool any_split = m != g->m;
    int max_sub = 0;
    for (const ResVCheck &v : vc) max_sub = std::max(max_sub, v.dc);
    std::vector<int> perm_v(n), pos_v(n);
    for (int j = 0; j < n; ++j) perm_v[j] = j;
    auto dv_of = [&](int j) { return g->h_var_ptr[j + 1] - g->h_var_ptr[j]; };
    std::stable_sort(perm_v.begin(), perm_v.end(), [&](int a, int b) { return dv_of(a) > dv_of(b); });
    std::vector<int> slot_of_edge(g->E);
    for (int p = 0; p < m; ++p)
        for (int t = 0; t < vc[p].dc; ++t) slot_of_edge[vc[p].e0 + t] = t * mstride + p;
    if (cl) {
        perm_v = cl->var_at;                                     // position -> variable, -1 = empty
        slot_of_edge = cl->slot_of_edge;                         // rows of a check in the placement's order
    } else {   // slots are fixed by the check order alone; choose the variable order inside each degree class
        std::vector<std::vector<int>> vs(n);
        for (int j = 0; j < n; ++j)
            for (int k = 0; k < dv_of(j); ++k) vs[j].push_back(slot_of_edge[g->h_csc[g->h_var_ptr[j] + k]]);
        optimise_lane_order(perm_v, vs, G);
    }
    const int n_pos = (int)perm_v.size();
    // the compact kernels load the plan entries of whole cells: padded to a multiple of 64 positions
    const int n_ent = cl ? (n_pos + 63) / 64 * 64 : n;
    for (int q = 0; q < n_pos; ++q)
        if (perm_v[q] >= 0) pos_v[perm_v[q]] = q;

    PlanTables pl;
    pl.dc_s.assign(m, 0); pl.gsz.assign(m, 0);
    pl.cvar.assign((size_t)S, 0); pl.bslot.assign((size_t)S, 0); pl.oaslot.assign((size_t)S, 0);
    pl.bslot_c.assign(m, 0); pl.inv_perm_v.assign(n, 0);
    pl.vmeta.assign(n_ent, 0u);
    pl.vslot_lo.assign(n_ent, Word2{0, kResHole}); pl.vslot_hi.assign(std::max(n_ent, 1), Word2{0, 0});
    int n_hi = 0;
    pl.edge_of_slot.assign((size_t)S, 0xffffffffu);
    pl.has_oaslot = in.form == kPlanOMS && in.has_oms_alpha;
    bool per_check = true;
    for (int p = 0; p < m; ++p) {
        const ResVCheck &v = vc[p];
        const int first = g->h_check_ptr[v.check];                  // the WHOLE check's first edge decides "one beta per check"
        pl.dc_s[p] = (uint8_t)v.dc;
        pl.gsz[p] = (uint8_t)v.gs;
        for (int t = 0; t < v.dc; ++t) {
            const int e = v.e0 + t, slot = slot_of_edge[e];
            pl.edge_of_slot[slot] = (uint32_t)e;
            pl.cvar[slot] = (uint16_t)pos_v[g->h_var_idx[e]];
            pl.bslot[slot] = (uint16_t)in.beta_slot[e];
            if (in.beta_slot[e] != in.beta_slot[first]) per_check = false;
            if (pl.has_oaslot) pl.oaslot[slot] = (uint16_t)in.oms_alpha_slot[e];
        }
        pl.bslot_c[p] = v.dc ? (uint16_t)in.beta_slot[first] : 0;
    }
    for (int q = 0; q < n_pos; ++q) {
        if (perm_v[q] < 0) continue;                                                   // empty: vmeta 0, kResHole
        const int j = perm_v[q], s0 = g->h_var_ptr[j], dv = dv_of(j);
        pl.vmeta[q] = (uint32_t)dv | ((uint32_t)in.alpha_slot[j] << 8);
        pl.inv_perm_v[j] = (uint16_t)q;
        uint32_t off[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int k = 0; k < dv; ++k) off[k] = (uint32_t)slot_of_edge[g->h_csc[s0 + k]] * G * 4;
        pl.vslot_lo[q] = Word2{off[0] | (off[1] << 16), off[2] | (off[3] << 16)};        // offsets <= 65535 (resident_fits)
        pl.vslot_hi[q] = Word2{off[4] | (off[5] << 16), off[6] | (off[7] << 16)};
        if (dv > 4) n_hi = q + 1;            // general plan: they come first; compact: all in round 0 (q < 512)
    }
    pl.n = n; pl.m = m; pl.S = (int)S; pl.max_dc = max_sub; pl.max_dv = g->max_dv; pl.mstride = mstride; pl.E = g->E;
    pl.any_split = any_split ? 1 : 0;
    pl.n_hi = n_hi;
    pl.n_pos = n_pos;
    pl.per_check = per_check;
    if (cl) {
        std::copy(cl->cell, cl->cell + kCptWaves, pl.vcell);
        cpt_check_words(vc, per_check && (in.form == kPlanNMS || (in.form == kPlanRCQ && in.rcq_zero0)), pl.ccell);
    }
    pl.par_words = is_pow2(mstride) ? m : 0;
    pl.par_shift = G == 2 ? 3 : 2;                     // slot byte offset = slot * G * 4
    pl.vslot_hi.resize((size_t)std::max(n_hi, 1));
    return pl;
}

// what a decoder gets on the LDS-resident engine: the general plan (G codewords per workgroup of NT threads, res_lds bytes
// of LDS) when res_ok, and the compact fixed-T plan with its grid when resc_ok
struct ResidentChoice {
    bool res_ok = false, resc_ok = false;
    int G = 0, NT = 0;
    size_t res_lds = 0, resc_lds = 0;
    PlanTables res, resc;
    CptLayout resc_layout;
};

// Sort checks and variables by degree (stable, descending), lay the edges out ELL-transposed.
inline ResidentChoice choose_resident_plan(const HostGraph *g, const PlanInputs &in)
{
    ResidentChoice c;
    if (g->E == 0 || g->max_dv > 8) return c;
    // fp64 (the reference's BasicMinSumDecoder dtype): the normalised form with one factor per check; a codeword's
    // 8-byte slots take the place of a float codeword PAIR, so the geometry below must come out at G = 2
    const bool f64 = in.dtype == kPlanF64;
    if (f64 && (in.form != kPlanNMS || !in.beta_per_check)) return c;
    const int n = g->n;
    if (n > 65535 || in.n_beta > 65535 || in.n_alpha >= (1 << 24) || in.n_oms_alpha > 65535) return c;

    std::vector<ResVCheck> vc;
    if (!resident_checks(g, vc)) return c;
    const int m = (int)vc.size();
    int max_sub = 0;
    for (const ResVCheck &v : vc) max_sub = std::max(max_sub, v.dc);
    if (m > 65535 || max_sub > 255) return c;

    // geometry: G codewords per workgroup, NT threads, and the row stride of the slot layout.
    // Two 512-thread workgroups per CU (G = 2, ds_read/write_b64) let one workgroup's barrier wait overlap
    // the other's phase -- measured best on the (1998,1512) code; larger codes fall back to one workgroup
    // per CU or G = 1.  A row stride of 512 slots (instead of m) lets LDS instructions carry t*stride as an
    // immediate offset; it is taken when it costs neither G nor workgroups per CU.
    auto geometry = [&](int stride, int &G_out, int &blocks_out) {
        const long long S_ = (long long)max_sub * stride;
        const int mp = is_pow2(stride) ? m : 0;           // parity words of the early-stop syndrome (power-of-two strides)
        if (S_ > 65535 || !resident_fits(in, n, S_, 1, 1, mp)) return false;
        const int G_ = resident_fits(in, n, S_, 2, 1, mp) ? 2 : 1;
        int b_ = 1;
        while (b_ < 8 && resident_fits(in, n, S_, G_, b_ + 1, mp)) ++b_;
        G_out = G_; blocks_out = b_;
        return true;
    };
    int G = 0, blocks = 0, mstride = m;
    if (!geometry(m, G, blocks)) return c;
    if (f64 && G != 2) return c;
    if (m <= 512) {
        int G5 = 0, b5 = 0;
        if (geometry(512, G5, b5) && G5 == G && std::min(b5, 2) == std::min(blocks, 2)) { mstride = 512; blocks = b5; }
    }
    const long long S = (long long)max_sub * mstride;
    c.res = resident_layout(g, in, vc, mstride, S, G);
    c.G = G; c.NT = blocks >= 2 ? 512 : 1024;
    c.res_lds = res_lds_total((int)S, n, G, resident_alpha_floats(in.dtype, in.T, in.n_alpha), c.res.par_words);
    c.res_ok = true;

    // compact fixed-T geometry: row stride kResCptStride, S truncated after the last slot in use (checks are sorted by
    // descending degree, so the last row holds only the checks of the largest degree), no llr_s / bits_s / parity words /
    // alpha table in LDS.  Taken when it gives kResCptBlocks workgroups of 512 threads per CU and the variable state fits
    // the registers (the engine's resident_reg_state)
    long long Sc = 0;
    if (!f64 && G == 2 && c.NT == kResCptThreads && cpt_geometry(g, vc, Sc)) {
        cpt_layout(g, vc, Sc, c.resc_layout);
        c.resc = resident_layout(g, in, vc, kResCptStride, Sc, 2, &c.resc_layout);
        c.resc_lds = res_cpt_lds_total((int)Sc, 2);
        c.resc_ok = true;
    }
    return c;
}

}  // namespace ldpc
