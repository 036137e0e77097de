// ldpc_resident_geom.h -- geometry of the LDS-resident engine that the kernels (ldpc_resident.hip) and the host planner
// (ldpc_plan.h) must agree on: sizes, the LDS carve and the encodings of the plan's cell and check words.  Plain C++17:
// the planner and its host test include it without a GPU toolchain.
#pragma once

#include <cstddef>

#if defined(__HIPCC__)
#define LDPC_HD __host__ __device__
#else
#define LDPC_HD
#endif

namespace ldpc {

constexpr size_t kLdsBytes = 160 * 1024;          // LDS per CU; one workgroup may take all of it
constexpr int kResSubDegreeCap = 32;              // checks up to this degree stay whole in the resident engine ...
constexpr int kResSubDegree = 16;                 // ... wider ones are split into lane groups of sub-checks this long

constexpr int kResAlphaMax = 1024;   // floats of alpha table kept in LDS

// Compact plan: the checks of wave w, one word of ResidentPlan::ccell (checks are sorted by degree, so nearly every wave
// holds one degree or two adjacent ones): d_lo = smallest degree in the wave | (largest - d_lo) << 8 | lanes in use << 16,
// kChkPerLane set for a wave the scalar-counted form does not take: d_lo < 4 (which also keeps the degree-1 rule
// "min2 = min1" in the per-lane form alone), and every wave of a decoder whose check phase is not the one-beta-per-check
// select form (per-edge beta, OMS, RCQ with tau_0 != 0).
constexpr unsigned kChkPerLane = 0x80000000u;
LDPC_HD constexpr unsigned chk_word(int d_lo, int d_hi, int lanes)
{
    return (unsigned)d_lo | (unsigned)(d_hi - d_lo) << 8 | (unsigned)lanes << 16 | (d_lo < 4 ? kChkPerLane : 0u);
}
LDPC_HD constexpr int chk_lo(unsigned w) { return (int)(w & 0xffu); }
LDPC_HD constexpr int chk_spread(unsigned w) { return (int)(w >> 8 & 0xffu); }
LDPC_HD constexpr int chk_lanes(unsigned w) { return (int)(w >> 16 & 0xffu); }

// variables a lane keeps in registers (ResVarState): the rounds of one variable phase of the REG and compact kernels
constexpr int kResRegVars = 4;

// Compact plan (CPT): the host places variables on a grid q = r*512 + w*64 + lane (round r, wave w) so that most
// (wave, round) cells hold ONE degree, and the cell table ResidentPlan::vcell tells every wave what its rounds hold:
constexpr unsigned kCellEmpty = 0x00;   // no variable: the round is skipped
constexpr unsigned kCellHoles = 0x40;   // | degree: one degree, some lanes empty (their vslot_lo.y is kResHole)
constexpr unsigned kCellMixed = 0xff;   // several degrees (or degree 0): the per-lane switch, degree from vmeta
                                        // otherwise the byte is the degree 1..8 of all 64 lanes
constexpr unsigned kResHole = 0xffffffffu;   // vslot_lo.y of an empty position (no variable's: offsets are multiples of 8)

// LDS carve (bytes): msg at 0, then llr_s, alpha_s, bits_s, the syndrome word
LDPC_HD inline size_t res_off_llr(int S, int G) { return (size_t)S * G * 4; }
LDPC_HD inline size_t res_off_alpha(int S, int n, int G) { return res_off_llr(S, G) + (size_t)n * G * 4; }
LDPC_HD inline size_t res_off_bits(int S, int n, int G, int n_alpha_lds) { return res_off_alpha(S, n, G) + (size_t)n_alpha_lds * 4; }
LDPC_HD inline size_t res_off_flag(int S, int n, int G, int n_alpha_lds) { return (res_off_bits(S, n, G, n_alpha_lds) + n + 3) / 4 * 4; }
LDPC_HD inline size_t res_off_par(int S, int n, int G, int n_alpha_lds) { return res_off_flag(S, n, G, n_alpha_lds) + 16; }
// `m_par` parity words follow (early-stop syndrome by scatter); 0 when the stride is not a power of two
LDPC_HD inline size_t res_lds_total(int S, int n, int G, int n_alpha_lds, int m_par) { return res_off_par(S, n, G, n_alpha_lds) + 4 * (size_t)m_par; }

// compact kernels (CPT): only the message slots and the flag words -- the LLR rows are staged in the not-yet-initialised
// message area and the posteriors in the dead one, the alpha table is read from global memory, no bits_s / parity words
LDPC_HD inline size_t res_cpt_off_flag(int S, int G) { return ((size_t)S * G * 4 + 15) / 16 * 16; }
LDPC_HD inline size_t res_cpt_lds_total(int S, int G) { return res_cpt_off_flag(S, G) + 16; }

// compact geometry (CPT): three 512-thread workgroups per CU -> six waves per SIMD, at most 80 VGPRs
constexpr int kResCptThreads = 512;
constexpr int kResCptWaves = 6;
constexpr int kResCptBlocks = 3;       // workgroups per CU the compact LDS carve must allow
// compile-time row stride of the compact slot layout (m <= 495).  Odd: with an even stride the bank of slot(p,t) =
// t*stride + p depends on p alone (496 = 0 mod 16 for the scatters) or on p and the parity of t (16 mod 32 for the
// gathers), so the rows give the host's placement search (cpt_place_banks) nothing to choose from.  495 and not 497: the
// (1998,1512) code at stride 496 takes 53,760 bytes of LDS, exactly a third of the CU's 128 allocation granules of 1,280
// bytes, and at 497 (53,856 bytes, under 160 KiB / 3 all the same) only two workgroups were resident per CU and the launch
// took 2.46 ms instead of 2.08 (profiles/README.md, r09).  The check phase is unaffected: consecutive p are consecutive
// 8-byte slots at any row base
constexpr int kResCptStride = 495;

}  // namespace ldpc
