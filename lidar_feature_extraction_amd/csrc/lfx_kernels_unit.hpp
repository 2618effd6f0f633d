// lfx_kernels_unit.hpp -- the unit kernels of the extraction path: one WAVE per (ring, block) unit, on the bucketed
// arrays (ring_unit_kernel) or on an organised scan's records in place (ring_unit_org_kernel).  Compiled once per
// VARIANT of the parameters (lfx_unit_variant.inl -> lfx_unit_v0.hip ... lfx_unit_v3.hip); overview: lfx_kernels_common.hpp.
#pragma once

#include "lfx_kernels_common.hpp"

#pragma clang fp contract(off)

namespace lfx
{

// ==========================================================================================
// Ring kernel, fast path: one WAVE per (ring, block) unit; no workgroup barrier anywhere.
//
// Unit j of a ring owns the output positions of block j (the first / last unit also own the ring's
// P-wide borders) and loads them with a halo of P+1 positions on either side: enough for the
// curvature window (P), the occlusion fills that can reach an owned point (P+1) and the
// parallel-beam test (1).  Lane l holds local positions q = 64k + l in registers; range and
// curvature also go to a wave-private LDS slab so that neighbours can be read by position.
// Rings the fast path cannot take (not angle-sorted as bucketed, skip conditions, blocks that do
// not fit a wave) are appended to `slow_list` and redone whole by ring_extract_kernel.
// Wave-uniform bit arrays in LDS.  A 64-bit ballot word per chunk, stored by the whole wave (every lane
// writes the same value to the same address, so each lane only ever reads back what it wrote itself:
// no fence is needed).  A lane then gets the 32 positions around its own one with one two-dword LDS
// read and one v_alignbit -- the words live neither in scalar registers (there are too few) nor in
// four selects per window.
enum { kBitLK, kBitJL, kBitJR, kBitA, kBitS, kBitSelE, kBitSelS, kUnitBitArrays };

// CH = chunks of 64 positions a unit may span (block + halo); the host picks the smallest that fits
// the longest ring it was configured for: less LDS and fewer registers per wave = more waves per CU.
template<int CH>
struct UnitLds
{
  static constexpr int kSpan = 64 * CH;
  static constexpr int kBitWords = 2 * (CH + 2);      // dwords per array; position p is bit p + 64
  // (the bit arrays come first and a pad last: the rows form of the window stages reads up to 2 CH values before r[0] and
  // behind the last c[] -- positions outside every block, whose results are thrown away -- and those reads stay inside the
  // wave's own slab)
  uint32_t bits[kUnitBitArrays][kBitWords];
  double r[kSpan];                                            // (organised-scan kernel: z of the hand-over until stage B)
  union {
    double c[kSpan + 2];                                      // from stage E on
    float2 pxy[kSpan + 2];                                    // stages A-C: x, y by position
  };
  // slab stride = 8 dwords mod 32: the four slabs of a workgroup start 8 LDS banks apart, so the hand-over stores of the
  // organised-scan kernel (16 lanes = 4 columns x 4 slabs, 8 bytes each) fall on 16 different bank pairs
  static constexpr int kBaseDwords = (kSpan * 8 + (kSpan + 2) * 8 + kUnitBitArrays * kBitWords * 4) / 4;
  static constexpr int kMinPadDwords = 2 * (2 * CH - 2);      // 2 CH - 2 doubles behind c[kSpan + 2]
  static constexpr int kPadDwords = ((8 - kBaseDwords % 32) + 32) % 32 + (((8 - kBaseDwords % 32) + 32) % 32 < kMinPadDwords ? 32 : 0);
  uint32_t pad_[kPadDwords];
};
static_assert(sizeof(UnitLds<5>) % 128 == 32 && sizeof(UnitLds<3>) % 128 == 32 && sizeof(UnitLds<4>) % 128 == 32 &&
  sizeof(UnitLds<6>) % 128 == 32 && sizeof(UnitLds<12>) % 128 == 32, "slab stride");
static_assert(7 * 4 * sizeof(UnitLds<5>) <= 160 * 1024 && 6 * 4 * sizeof(UnitLds<6>) <= 160 * 1024 && 8 * 4 * sizeof(UnitLds<4>) <= 160 * 1024,
  "workgroups per CU the launch bounds count on");
#ifndef LFX_UNIT_WAVES_CH5
#define LFX_UNIT_WAVES_CH5 7
#endif
#ifndef LFX_LIBRARY_SQRT
#define LFX_LIBRARY_SQRT 0
#endif
#ifndef LFX_COS_BAND
#define LFX_COS_BAND 0x1p-20f
#endif
// (variant 0, the headline's, keeps 7 workgroups per CU at 5 chunks in 72 registers without a spill; the other variants hold
// their thresholds in registers and get the 80 of 6 workgroups per CU -- 6 against 7 made no measurable difference, round 5)
// (... and so do the kernels that apply ring transforms in their loads: 8 spilled vector registers at 72.  6 chunks: 5
// workgroups per CU and 96 registers -- at 6 the kernel spilled 8 registers to scratch, and scratch traffic costs a kernel
// that is bound by its memory operations 5 %: 270 -> 284 k scans/s at 128 x 2048 x 32, round 5)
constexpr int unit_waves_per_simd(int ch, int variant = 0, bool xf = false)
{
  return ch > 6 ? 3 : (ch == 6 ? 5 : (ch == 5 ? (variant == 0 && !xf ? LFX_UNIT_WAVES_CH5 : 6) : (ch == 4 ? 7 : 8)));     // (4 chunks: 72 registers, no spills)
}

// LDS traffic of one wave is executed in order; this only stops the compiler from moving a
// lane's LDS read above another lane's LDS write of the same wave.
#define LFX_WAVE_SYNC() \
  do { \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
    __builtin_amdgcn_wave_barrier(); \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
  } while (0)

// A window of NW consecutive doubles from LDS, starting at `first`, as NW single ds_read_b64.  Left to itself the backend
// fuses the reads of a stencil pairwise into ds_read2_b64, which occupies the LDS pipe for 8 cycles where two
// ds_read_b64 take 2 each (MI355X_MICROARCH.md, LDS table) -- and the LDS pipe is this kernel's busiest resource
// (SQ_ACTIVE_INST_LDS x 28 waves per CU ~ a wave's whole life).  Inline asm: the reads are invisible to the
// compiler's own waits, so the wait is part of the sequence and carries every destination through it (no use of a
// value can be scheduled between its read and the wait).
template<int NW>
__device__ __forceinline__ void lds_window_f64(const double * first, double (&w)[NW])
{
  static_assert(NW <= 22, "extend the wait's operand list");
  const uint32_t addr = (uint32_t)reinterpret_cast<uintptr_t>(first);      // LDS byte address = low half of the generic one
#pragma unroll
  for (int i = 0; i < NW; i++) {
    asm volatile ("ds_read_b64 %0, %1 offset:%2" : "=v"(w[i]) : "v"(addr), "n"(8 * i));
  }
  // (the wait names exactly the NW destinations: operands that stand for nothing would each cost a register pair and a
  // v_mov to fill it -- nine of them per two-wide window, 135 vector instructions per wave, until round 4)
  if constexpr (NW == 2) {
    asm volatile ("s_waitcnt lgkmcnt(0)" : "+v"(w[0]), "+v"(w[1]));
  } else if constexpr (NW == 5) {
    asm volatile ("s_waitcnt lgkmcnt(0)" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(w[4]));
  } else if constexpr (NW == 11) {
    asm volatile ("s_waitcnt lgkmcnt(0)"
      : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(w[4]), "+v"(w[5]), "+v"(w[6]), "+v"(w[7]), "+v"(w[8]), "+v"(w[9]), "+v"(w[10]));
  } else if constexpr (NW == 15) {
    asm volatile ("s_waitcnt lgkmcnt(0)"
      : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(w[4]), "+v"(w[5]), "+v"(w[6]), "+v"(w[7]), "+v"(w[8]), "+v"(w[9]), "+v"(w[10]),
        "+v"(w[11]), "+v"(w[12]), "+v"(w[13]), "+v"(w[14]));
  } else if constexpr (NW == 16) {
    asm volatile ("s_waitcnt lgkmcnt(0)"
      : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(w[4]), "+v"(w[5]), "+v"(w[6]), "+v"(w[7]), "+v"(w[8]), "+v"(w[9]), "+v"(w[10]),
        "+v"(w[11]), "+v"(w[12]), "+v"(w[13]), "+v"(w[14]), "+v"(w[15]));
  } else {
    static_assert(NW == 1 || NW == 3 || NW == 7 || NW == 8 || NW == 9 || NW == 10 || NW == 13 || NW == 14 || NW == 22, "add the wait for this window width");
    if constexpr (NW == 8) {
      asm volatile ("s_waitcnt lgkmcnt(0)" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(w[4]), "+v"(w[5]), "+v"(w[6]), "+v"(w[7]));
    }
    if constexpr (NW == 10) {
      asm volatile ("s_waitcnt lgkmcnt(0)"
        : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(w[4]), "+v"(w[5]), "+v"(w[6]), "+v"(w[7]), "+v"(w[8]), "+v"(w[9]));
    }
    if constexpr (NW == 13) {
      asm volatile ("s_waitcnt lgkmcnt(0)"
        : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(w[4]), "+v"(w[5]), "+v"(w[6]), "+v"(w[7]), "+v"(w[8]), "+v"(w[9]), "+v"(w[10]),
          "+v"(w[11]), "+v"(w[12]));
    }
    if constexpr (NW == 22) {
      asm volatile ("s_waitcnt lgkmcnt(0)"
        : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(w[4]), "+v"(w[5]), "+v"(w[6]), "+v"(w[7]), "+v"(w[8]), "+v"(w[9]), "+v"(w[10]),
          "+v"(w[11]), "+v"(w[12]), "+v"(w[13]), "+v"(w[14]), "+v"(w[15]), "+v"(w[16]), "+v"(w[17]), "+v"(w[18]), "+v"(w[19]), "+v"(w[20]),
          "+v"(w[21]));
    }
    if constexpr (NW == 14) {
      asm volatile ("s_waitcnt lgkmcnt(0)"
        : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(w[4]), "+v"(w[5]), "+v"(w[6]), "+v"(w[7]), "+v"(w[8]), "+v"(w[9]), "+v"(w[10]),
          "+v"(w[11]), "+v"(w[12]), "+v"(w[13]));
    }
    if constexpr (NW == 1) {asm volatile ("s_waitcnt lgkmcnt(0)" : "+v"(w[0]));}
    if constexpr (NW == 3) {asm volatile ("s_waitcnt lgkmcnt(0)" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]));}
    if constexpr (NW == 7) {
      asm volatile ("s_waitcnt lgkmcnt(0)" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(w[4]), "+v"(w[5]), "+v"(w[6]));
    }
    if constexpr (NW == 9) {
      asm volatile ("s_waitcnt lgkmcnt(0)"
        : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(w[4]), "+v"(w[5]), "+v"(w[6]), "+v"(w[7]), "+v"(w[8]));
    }
  }
}

// Lane predicate <-> wave-uniform mask.  `bal` is meant for ONE comparison (it then is the
// comparison's own result register); combine masks with & | ~ in scalar code.
__device__ inline uint64_t bal(bool p) {return __builtin_amdgcn_ballot_w64(p);}
__device__ inline bool lanes(uint64_t m) {return __builtin_amdgcn_inverse_ballot_w64(m);}
// lanes whose position q lies in [lo, hi) (lo, hi wave-uniform): one subtract and one compare per lane --
// the scalar unit is as busy as the vector unit in this kernel, so the mask is not built from shifts
__device__ inline uint64_t in_span(int q, int lo, int hi)
{
  const int width = hi - lo;
  return bal((uint32_t)(q - lo) < (uint32_t)(width > 0 ? width : 0));
}

struct UnitWin
{
  uint32_t ofs, sh;      // dword offset of the window's first dword inside a chunk pair; bit shift
};

// (the bit arrays are dwords read back in pairs and written as 64-bit words: both accesses are declared may_alias --
// under the type-based aliasing rules a uint64_t store and a uint32_t load could otherwise be reordered, and in
// straight-line code they were: a lane then read the live set of the round before and the pick rounds never ended)
typedef uint64_t __attribute__((may_alias)) u64_alias_t;
typedef uint32_t __attribute__((may_alias)) u32_alias_t;
typedef float __attribute__((may_alias)) f32_alias_t;

template<int CH>
__device__ inline void put_word(UnitLds<CH> & U, int arr, int k, uint64_t w)
{
  *reinterpret_cast<u64_alias_t *>(&U.bits[arr][2 * (k + 1)]) = w;
}

// The words of one bit array, gathered in a register pair before they go to LDS: lane k + 1 holds the word of chunk k
// (lanes 0 and K + 1 ... the zero words on either side), so that the array is written by ONE ds_write_b64 instead of one
// per chunk -- a store of a wave-uniform word occupies the LDS pipe like any other (6 cycles), the pipe is the busiest
// resource of the kernel, and these stores were a third of its cycles.  v_writelane costs what the v_mov of the word
// into a register cost before.
struct WordVec
{
  uint32_t lo = 0u, hi = 0u;
  __device__ __forceinline__ void set(int k, uint64_t w)
  {
    // (clang has no builtin for v_writelane.  One scalar register per VALU instruction is all gfx9's constant bus allows,
    // so the lane select has to be a literal: k is a constant once the chunk loops are unrolled and the switch folds.
    // s_nop 1: on gfx940 and later a VALU instruction must not read a scalar register within two wait states of the VALU
    // instruction that wrote it -- the word is a v_cmp result as a rule -- and the compiler pads no hazard whose consumer
    // is inside an asm string: without the nop the OLD register value was written and the pick rounds never ended)
    const uint32_t wlo = __builtin_amdgcn_readfirstlane((uint32_t)w), whi = __builtin_amdgcn_readfirstlane((uint32_t)(w >> 32));
#define LFX_WRITELANE(L) \
  case L - 1: \
    asm ("s_nop 1\n\tv_writelane_b32 %0, %2, " #L "\n\tv_writelane_b32 %1, %3, " #L : "+v"(lo), "+v"(hi) : "s"(wlo), "s"(whi)); \
    break;
    switch (k) {
      LFX_WRITELANE(1) LFX_WRITELANE(2) LFX_WRITELANE(3) LFX_WRITELANE(4) LFX_WRITELANE(5) LFX_WRITELANE(6)
      LFX_WRITELANE(7) LFX_WRITELANE(8) LFX_WRITELANE(9) LFX_WRITELANE(10) LFX_WRITELANE(11) LFX_WRITELANE(12)
      default: break;
    }
#undef LFX_WRITELANE
    static_assert(kUnitMaxChunks <= 12, "one case per chunk");
  }
};

template<int CH>
__device__ __forceinline__ void put_words(UnitLds<CH> & U, int arr, const WordVec & v, int lane)
{
  // Lanes 0 .. CH + 1 store.  The execution mask is set inside the statement: written as `if (lane < CH + 2)` the
  // compiler (ROCm 7.2) placed window reads that FOLLOW the store inside the masked region, so that only those seven
  // lanes read their windows (seen in the listing; the pick rounds then never ended).  An LDS write the compiler does
  // not count only makes its own lgkmcnt waits conservative (LDS operations of a wave complete in order).
  const uint32_t addr = (uint32_t)reinterpret_cast<uintptr_t>(&U.bits[arr][0]) + 8u * (uint32_t)lane;
  const uint64_t data = ((uint64_t)v.hi << 32) | v.lo;
  uint64_t saved;
  asm volatile ("s_mov_b64 %0, exec\n\ts_mov_b64 exec, %3\n\tds_write_b64 %1, %2\n\ts_mov_b64 exec, %0"
    : "=&s"(saved) : "v"(addr), "v"(data), "n"((1u << (CH + 2)) - 1u) : "memory");
}

// bit 16 + d of the result <-> position q + d of array `arr`, q = 64k + lane (+1 for the shifted constants)
template<int CH>
__device__ inline uint32_t get_win(const UnitLds<CH> & U, int arr, int k, const UnitWin & w)
{
  const u32_alias_t * b = reinterpret_cast<const u32_alias_t *>(&U.bits[arr][2 * k + w.ofs]);
  return __builtin_amdgcn_alignbit(b[1], b[0], w.sh);
}

// 32 positions of array `arr` starting at position `first` (bit i of the result <-> position first + i), first >= -64
template<int CH>
__device__ inline uint32_t get_win_at(const UnitLds<CH> & U, int arr, int first)
{
  const uint32_t bit = (uint32_t)(first + 64);
  const u32_alias_t * b = reinterpret_cast<const u32_alias_t *>(&U.bits[arr][bit >> 5]);
  return __builtin_amdgcn_alignbit(b[1], b[0], bit & 31u);
}

// The ROWS form of the block labelling (unit_core, stages D and F).  A lane holds CH CONSECUTIVE positions, CH * lane + d,
// and every point set of the pick rounds is CH bits of one vector register per lane (bit d <-> position CH * lane + d).
// What a position needs to see -- PT positions either side -- lies in its own lane and the two lanes next to it (PT <= CH):
// the FRAME of a set is [the top PT bits of the lane below | the lane's own CH bits | the low PT bits of the lane above],
// bit i <-> position CH * lane - PT + i, put together from two wave-wide DPP shifts (wave_shr:1 / wave_shl:1 cross the
// rows of 16 lanes on gfx9; the wave's two ends read 0).  A round of the priority fix-point is then AND / MIN / shift-OR on
// registers: no ballot, no scalar mask, no LDS bit array -- the chunk form paid, per chunk and per round, a ballot, scalar
// logic, two v_writelane, an LDS store and an LDS read back (round 4's per-wave counters: 1 086 scalar and 179 LDS
// instructions, the scalar file at 94 registers).
__device__ __forceinline__ uint32_t from_lane_below(uint32_t v) {return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xF, 0xF, true);}   // wave_shr:1
__device__ __forceinline__ uint32_t from_lane_above(uint32_t v) {return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xF, 0xF, true);}   // wave_shl:1

template<int CH, int PT>
__device__ __forceinline__ uint32_t row_frame(uint32_t own)
{
  static_assert(PT >= 1 && PT <= 2 * CH && (PT > CH ? 3 * CH + PT : 2 * CH + PT) <= 32,
    "the halo of a lane's positions must lie in the two lanes either side of it, the frame in one register");
  const uint32_t below = from_lane_below(own), above = from_lane_above(own);
  uint32_t f = (own << PT) | (above << (PT + CH));                   // (bits beyond the frame's CH + 2 PT meet no mask)
  if constexpr (PT >= CH) {f |= below << (PT - CH);} else {f |= below >> (CH - PT);}
  if constexpr (PT > CH) {
    f |= from_lane_below(below) >> (2 * CH - PT);
    f |= from_lane_above(above) << (PT + 2 * CH);
  }
  return f;
}

// bit d of the result <-> the frame meets mask[d]
template<int CH>
__device__ __forceinline__ uint32_t row_hits(uint32_t frame, const uint32_t (&mask)[CH])
{
  uint32_t h = 0;
#pragma unroll
  for (int d = 0; d < CH; d++) {
    const uint32_t t = frame & mask[d];
    h |= (t < 1u ? t : 1u) << d;
  }
  return h;
}

// which lane holds position q of the rows form, q < 64 * CH: q / CH by one 24-bit multiply (checked for every q below)
template<int CH> struct RowDiv { static constexpr uint32_t kShift = 18, kMul = ((1u << 18) + CH - 1) / CH; };
template<int CH> constexpr bool row_div_exact()
{
  for (uint32_t q = 0; q < 64u * CH; q++) {
    if (((q * RowDiv<CH>::kMul) >> RowDiv<CH>::kShift) != q / CH) {return false;}
  }
  return true;
}

// sqrt of a sum of two squares of floats, in f64, correctly rounded (math.hpp:36-39: std::sqrt of the double sum).  The
// library's sqrt scales its argument first, for values below 2^-767 -- which x * x + y * y of two floats never is (zero, or
// at least 2^-298: the square of the smallest subnormal float) -- so its own iteration is used without the scaling: the
// reciprocal-square-root estimate, one coupled Goldschmidt step and two corrections of the root by its residual, each
// fused (an explicit fma: only implicit contraction is off).  Seven instructions fewer per 64 points than sqrt().
__device__ __forceinline__ double sqrt_sum_of_squares(double a)
{
#if LFX_LIBRARY_SQRT
  return sqrt(a);
#else
  const double y0 = __builtin_amdgcn_rsq(a);
  double g = a * y0, h = 0.5 * y0;
  const double r0 = __builtin_fma(-h, g, 0.5);
  g = __builtin_fma(g, r0, g);
  h = __builtin_fma(h, r0, h);
  const double d0 = __builtin_fma(-g, g, a);
  g = __builtin_fma(d0, h, g);
  const double d1 = __builtin_fma(-g, g, a);
  g = __builtin_fma(d1, h, g);
  // +0 and +infinity are their own roots (the estimate is infinite / zero there), a NaN stays one
  return __builtin_amdgcn_class(a, 0x260) ? a : g;
#endif
}

// Branch-free form of polar_less for the common case, as masks: `spec` = one of the predicate's
// special cases may apply (equal points, a zero point, a point on the x axis) and the full predicate
// has to be evaluated instead.
__device__ inline uint64_t polar_less_masks(float ax, float ay, float bx, float by, uint64_t & spec, const float tiny = 1e-18f)
{
  // a SUPERSET of the special cases is enough (the caller re-evaluates flagged pairs with the full
  // predicate): |y| < 1e-18 covers y == 0 and every point whose squared length rounds (or flushes) to
  // zero in f32, which needs |x|, |y| < 1.1e-19
  spec = (bal(ax == bx) & bal(ay == by)) | bal(fabsf(ay) < tiny) | bal(fabsf(by) < tiny);
  const float det = ax * by - ay * bx;
  const uint64_t same = bal(ay * by > 0.f);
  return (same & bal(det > 0.f)) | (~same & bal(ay < 0.f));
}

// Stage ablations of the unit kernel (tools/ablate.sh) exist in the diagnostic build only (-DLFX_ABLATE, `make
// ablate`): LFX_DEBUG_UNIT_FLAGS then switches stages off (bits 256 occlusion, 512 parallel beam, 1024 records;
// bits 1 / 64 = edge / surface pass kept).  The product build has no such tests in its instruction stream.
#ifdef LFX_ABLATE
#define LFX_STAGE_ON(bit) (!(dbg_flags & (bit)))
#define LFX_STAGE_KEPT(bit) ((dbg_flags & (bit)) != 0u)
#else
#define LFX_STAGE_ON(bit) true
#define LFX_STAGE_KEPT(bit) true
#endif

// Diagnostic build only (-DLFX_STAMPS): shader-clock stamps at the stage boundaries of the unit kernel,
// kept for the first kStampUnits units of scan LFX_STAMP_SCAN; read back with lfx_debug_read_stamps.  The product
// build executes none of this.
#ifdef LFX_STAMPS
#ifndef LFX_STAMP_SCAN
#define LFX_STAMP_SCAN 128
#endif
constexpr int kStampSlots = 16, kStampUnits = 384;
static __device__ unsigned long long g_unit_stamps[kStampUnits * kStampSlots];     // (one per translation unit: the reader sits with variant 0's kernels)
// (stamps 0 and 10 also leave the constant-rate REFCLK counter, which all CUs share, in slots 11 and 12: when the units of a
// scan start and end against one another, tools/stamps.py --skew)
#define LFX_STAMP(n) \
  do { \
    if (s == (uint32_t)LFX_STAMP_SCAN && (uint32_t)(slot * B + j) < (uint32_t)kStampUnits) { \
      const unsigned long long t_ = __builtin_amdgcn_s_memtime(); \
      if (lane == 0) {g_unit_stamps[(slot * B + j) * kStampSlots + (n)] = t_;} \
      if ((n) == 0 || (n) == 10) { \
        const unsigned long long r_ = __builtin_amdgcn_s_memrealtime(); \
        if (lane == 0) {g_unit_stamps[(slot * B + j) * kStampSlots + ((n) == 0 ? 11 : 12)] = r_;} \
      } \
    } \
  } while (0)
#elif defined(LFX_MARKS)
// Diagnostic assembly only (make marks): a comment line at every stage boundary, so that the instructions of the
// listing can be counted per stage (tools/count_stage_instructions.py).
#define LFX_STAMP(n) asm volatile ("; LFX_MARK " #n ::: "memory")
#else
#define LFX_STAMP(n) do {} while (0)
#endif

// ORG: the organised-scan form.  A driver's scan arrives column-major -- all rings of one firing, then the next
// azimuth -- so that ring r's position k IS input point k * R + r (R = the sensor's ring count) and the rings are
// angle-sorted as they stand.  Then nothing needs bucketing: the workgroup's four waves take the same block of four
// ADJACENT rings and load the 32-byte records themselves, lane = (column, ring of the group), so that every 128-byte
// line (one column of the four rings) is requested once by four neighbouring lanes; x, y (and z) are handed to the
// ring's wave through its LDS slab (the workgroup's only barrier).  The pattern -- ring id of every record, point
// count, angle order -- is verified on the way; a scan that breaks it is flagged and redone whole by the bucketing
// route (scan_falls_back).  MakePointIndices / SortEachRingByAngle (ring.hpp:114-139) give exactly this order for
// such a scan: arrival order inside a ring, which is already the angle order.
struct OrgScan
{
  const uint8_t * __restrict__ pts;       // canonical 32-byte PointXYZIR records (point_type.hpp:62-86)
  const uint32_t * __restrict__ scan_begin;
  uint32_t * __restrict__ ring_count_out;
  uint32_t R, r0, wave, drop_zero;
  const uint32_t * __restrict__ xform;    // [batch][256] ring transforms (XF instantiations only)
  const uint32_t * __restrict__ geom;     // [batch][kGeomStride]
};

// (The FULL form of the body -- every chunk processed whatever the span, no chunk skipped, so that a stage is straight-line code --
// was an experiment of round 2: 1 700 against 1 440 us, 42 scalar and 24 vector registers spilled.  It exposed the aliasing hazard
// described at put_word() and was taken out in round 5: git show 238d4cf:lidar_feature_extraction_amd/csrc/lfx_kernels_unit.hpp.)
// What a unit is, in ring positions i and in span coordinates q = i - g0 (wave-uniform, scalar registers).
struct UnitGeom
{
  int N, b0, b1, o0, o1, g0, span, K, qb0, qb1, qo0, qo1, qlo, qhi;
};

__device__ inline UnitGeom unit_geometry(int N, int P, int B, int j, int b0, int b1)
{
  UnitGeom G;
  G.N = N; G.b0 = b0; G.b1 = b1;
  G.o0 = j == 0 ? 0 : b0; G.o1 = j == B - 1 ? N : b1;
  const int H = P + 1;
  G.g0 = G.o0 - H; G.span = G.o1 + H - G.g0;
  G.K = (G.span + 63) >> 6;
  G.qb0 = b0 - G.g0; G.qb1 = b1 - G.g0;          // the block in span coordinates
  G.qo0 = G.o0 - G.g0; G.qo1 = G.o1 - G.g0;      // the owned positions
  G.qlo = G.g0 < 0 ? -G.g0 : 0;                  // first / one-past-last position that is a ring point
  G.qhi = (N - G.g0) < G.span ? (N - G.g0) : G.span;
  return G;
}

// Stages B-G of a unit (see unit_body): x, y (zero outside the ring) are in registers AND in the wave's slab (U.pxy), z
// in registers.  Returns 0, or the reason the unit cannot be taken here (kDeferOrder / kDeferOther); feature records go
// to positions [rec_lo, ...) (edges, ascending) and (..., rec_hi) (surfaces, descending) of the ring's record arrays,
// their numbers to n_edge / n_surface.
template<int PT, int CH, bool DEF, bool ORG, bool XF, bool SIDX = false>
__device__ __forceinline__ uint32_t unit_core(
  const Params & prm, UnitLds<CH> & U, const UnitGeom & G, uint32_t dbg_flags, uint32_t s, uint32_t slot, int j,
  const float (&x)[CH], const float (&y)[CH], const float (&z)[CH], const uint32_t (&src)[CH],
  const UnitTables * __restrict__ tab, bool second_pass, const OrgScan & og, size_t off, uint32_t max_rings,
  uint32_t rec_lo, uint32_t rec_hi, uint32_t & n_edge, uint32_t & n_surface, const int lane)
{
  const int P = PT > 0 ? PT : prm.P, B = prm.B;
  (void)B;
  // DEF: the thresholds are the reference's code defaults (hyper_parameter.hpp:35-43; the host checks) and become
  // literals: seven fewer long-lived scalar values in a kernel that spills scalar registers (-3.4 % time)
  // (!DEF: the thresholds come from the copy of the parameter block behind `tab`, fetched where a stage first needs them
  // -- as kernel arguments they sat in nineteen scalar registers from the first instruction to the last)
  const int N = G.N, o0 = G.o0, o1 = G.o1, g0 = G.g0, span = G.span, K = G.K;
  const int qb0 = G.qb0, qb1 = G.qb1, qo0 = G.qo0, qo1 = G.qo1, qlo = G.qlo, qhi = G.qhi;
  (void)o0; (void)o1;
  const UnitWin W0{(uint32_t)(lane + 48) >> 5, (uint32_t)(lane + 16) & 31u};   // window around q
  const UnitWin W1{(uint32_t)(lane + 49) >> 5, (uint32_t)(lane + 17) & 31u};   // window around q + 1
  // The masks that override the block labelling (feature_extraction.cpp:133-138), three bits per chunk in one register:
  // they are known long before the labels (stages C and D, where the ranges and the jumps are at hand), and as wave-
  // uniform masks they would hold 3 x CH scalar pairs through the pick rounds
  constexpr uint32_t kOvrOccluded = 1u, kOvrRange = 2u, kOvrBeam = 4u;
  uint32_t ovr[(CH + 9) / 10];                  // (ten chunks to a register)
#pragma unroll
  for (int t = 0; t < (CH + 9) / 10; t++) {ovr[t] = 0;}
  LFX_STAMP(2);
  // ---- B. range (math.hpp:36-39)
#pragma unroll
  for (int k = 0; k < CH; k++) {
    if (k < K) {
      const int q = 64 * k + lane;
      const double xd = (double)x[k], yd = (double)y[k];
      U.r[q] = sqrt_sum_of_squares(xd * xd + yd * yd);     // (kept in the slab only: registers are what the straight-line form is short of)
    }
  }
  LFX_WAVE_SYNC();
  LFX_STAMP(3);
  // ---- C. angle order of the owned pairs (ring.hpp:54-112): strictly increasing as bucketed, else slow path; links
  //         (neighbor.hpp:44-48): bit q <-> pair (q, q+1); with them the range jumps of the occlusion test
  //         (occlusion.hpp:44-57, 67-79)
  {
    // (one walk over the chunks, one read of the neighbour's x, y for the order test and the link's dot product; a
    // chunk's links are final -- the undecided ones settled by the exact division at once -- before its jumps are taken
    // from the same two ranges)
    asm volatile ("" ::: "memory");
    const double dist_diff = DEF ? 0.3 : tab->prm.dist_diff;
    const double min_range = DEF ? 0.1 : tab->prm.min_range, max_range = DEF ? 100.0 : tab->prm.max_range;
    const double pb_ratio = DEF ? 0.02 : tab->prm.pb_ratio;
    const float pb_ratio_f = DEF ? 0.02f : tab->prm.pb_ratio_f;
    const double cos_bound = tab->prm.cos_bound;
    const int pair_end = qo1 < qhi - 1 ? qo1 : qhi - 1;                // owned pairs (q, q+1): q in [qo0, pair_end)
    uint64_t bad = 0;
    uint64_t zero_pair = 0;
    uint64_t prev_top = 0;                               // link of the pair (64k - 1, 64k)
    WordVec vlk, vjl, vjr;
    const float cbf = tab->prm.cos_bound_f;
    // parallel_beam.hpp:43-49: (float)(|dr| / r) > ratio on both sides.  f32 pre-filter: the
    // differences of the f32 ranges are within 2 ulp(r) of the exact ones, i.e. within
    // 2^-22 * r; against the threshold ratio * r that is a relative error of 2^-22 / ratio, so a
    // band of 2^-12 around the threshold is safe for any ratio >= 2^-9 (smaller ratios: exact path).
    const bool ratio_ok = pb_ratio_f >= 0x1p-9f;
    // The constants of this walk, held in vector registers: a comparison into a scalar pair takes no literal, and a
    // 64-bit one never, so every use of a literal was one or two scalar moves -- sixteen per chunk; the scalar unit is as
    // busy as the vector unit here and its registers are all taken, the vector file has a few to spare in this stage.
    double c_dd = dist_diff, c_min = min_range, c_max = max_range;
    float c_one_lo = 1.0f - LFX_COS_BAND, c_one_hi = 1.0f + LFX_COS_BAND, c_tiny = 1e-18f, c_big = 1e30f, c_zero = 0.f, c_small = 1e-30f;
    asm volatile ("" : "+v"(c_dd), "+v"(c_min), "+v"(c_max), "+v"(c_one_lo), "+v"(c_one_hi), "+v"(c_tiny), "+v"(c_big), "+v"(c_zero), "+v"(c_small));
#pragma unroll
    for (int k = 0; k < CH; k++) {
      if (k < K) {
        const int q = 64 * k + lane;
        const uint64_t pair = in_span(q, qlo, qhi - 1);
        // the neighbour's x, y and the three ranges r[q - 1], r[q], r[q + 1] behind ONE wait (position 0 has no left
        // neighbour: its window starts at itself)
        const float2 nb = U.pxy[q + 1];
        double rw3[3];
        lds_window_f64(&U.r[k == 0 ? (q > 0 ? q - 1 : 0) : q - 1], rw3);
        double rk = rw3[1], rn = rw3[2];
        const double rm = rw3[0];                  // (r[0] for position 0, as the clamped read gave)
        if (k == 0) {
          rk = q == 0 ? rw3[0] : rk;
          rn = q == 0 ? rw3[1] : rn;
        }
        zero_pair |= pair & in_span(q, qo0, qo1) & bal(rk == 0.) & bal(rn == 0.);       // math.cpp:40-42 throws
        // cos_bound <= cos <= 1 (neighbor.hpp:44-48 via the cosine bound): classified in f32 first.  With r0 r1 in
        // [1e-30, 1e30] (no product below the normal range matters, nothing overflows) the f32 cosine is within
        // 9 x 2^-24 = 5.4e-7 of the exact one: |x0 x1|, |y0 y1| <= r0 r1, so two products and their sum err by 3 x 2^-24
        // of r0 r1; the two converted ranges and their product by 3 x 2^-24 of it, the reciprocal by one ulp, the last
        // product by half of one; the bound itself was rounded to f32 (6e-8).  A value more than 2^-20 (9.5e-7) away from
        // both ends decides the test, anything closer -- or outside that range, or not a number -- takes the exact f64
        // division.  (2^-19 until round 4: at 3 600 columns neighbours are 1.5e-6 below cos = 1 and every pair took the
        // division.)
        {
          uint64_t spec;
          const uint64_t less = polar_less_masks(x[k], y[k], nb.x, nb.y, spec, c_tiny);
          bad |= in_span(q, qo0, pair_end) & (spec | ~less);
        }
        const float dotf = x[k] * nb.x + y[k] * nb.y;
        const float denf = (float)rk * (float)rn;
        const float cosf = dotf * __builtin_amdgcn_rcpf(denf);
        const uint64_t yes = bal(cosf > cbf + LFX_COS_BAND) & bal(cosf < c_one_lo);
        const uint64_t no = bal(cosf < cbf - LFX_COS_BAND) | bal(cosf > c_one_hi);
        const uint64_t fin = bal(denf > c_small) & bal(denf < c_big);
        uint64_t lk = yes & ~no & fin & pair;
        const uint64_t undecided = (~(yes | no) | ~fin) & pair;
        if (undecided != 0ull) {
          const double dot = (double)x[k] * (double)nb.x + (double)y[k] * (double)nb.y;
          const double cosang = dot / (rk * rn);                         // math.cpp:44-45
          lk |= undecided & bal(cosang >= cos_bound) & bal(cosang <= 1.0);    // acos(cos) < threshold; NaN -> false
        }
        vlk.set(k, lk);
        const double rq = rk + c_dd;
        // far side to the right of a linked pair (q, q+1), i in [0, N-P-1)
        const uint64_t jl = lk & in_span(q, 0, N - P - 1 - g0) & bal(rn > rq);
        // far side to the left of a linked pair (q-1, q), i in [P+1, N-1]
        const uint64_t lk_prev = (lk << 1) | prev_top;
        const uint64_t jr = lk_prev & in_span(q, P + 1 - g0, qhi) & bal(rm > rq);
        prev_top = lk >> 63;
        if (LFX_STAGE_ON(256u)) {
          vjl.set(k, jl);
          vjr.set(k, jr);
        }
        // the range test (range.hpp:40-43) and the parallel-beam test of position q, from the same three ranges; the
        // latter settled by the exact division at once where the f32 test leaves it open
        uint64_t pb = 0;
        if (LFX_STAGE_ON(512u)) {
          const float rf = (float)rk, rmf = (float)rm, rpf = (float)rn;
          const float a1 = fabsf(rmf - rf), a2 = fabsf(rpf - rf);
          const float thr = pb_ratio_f * rf;
          const float hi_t = thr * (1.0f + 0x1p-12f), lo_t = thr * (1.0f - 0x1p-12f);
          const uint64_t guard = ratio_ok ? (bal(rf > c_zero) & bal(rf < c_big)) : 0ull;
          // decided yes: both sides clearly above the threshold; decided no: one side clearly below it; anything else (and
          // everything outside the guard) takes the exact division
          const uint64_t yy = bal(a1 > hi_t) & bal(a2 > hi_t) & guard;
          const uint64_t nn = (bal(a1 < lo_t) | bal(a2 < lo_t)) & guard;
          // i in [1, N-1) and owned
          const uint64_t valid = in_span(q, 1 - g0, N - 1 - g0) & in_span(q, qo0, qo1);
          pb = yy & valid;
          const uint64_t undecided = valid & ~(yy | nn);
          if (undecided != 0ull) {
            const float ratio1 = (float)(fabs(rm - rk) / rk);
            const float ratio2 = (float)(fabs(rn - rk) / rk);
            pb |= undecided & bal((double)ratio1 > pb_ratio) & bal((double)ratio2 > pb_ratio);
          }
        }
        const uint64_t oor = ~(bal(c_min <= rk) & bal(rk <= c_max));                  // (a NaN range is out of range)
        ovr[k / 10] |= (lanes(oor) ? (uint32_t)kOvrRange << (3 * (k % 10)) : 0u) | (lanes(pb) ? (uint32_t)kOvrBeam << (3 * (k % 10)) : 0u);
      }
    }
    if (bad != 0ull) {
      // re-evaluate with the full predicate: a special case is not necessarily out of order
      bool really = false;
#pragma unroll
      for (int k = 0; k < CH; k++) {
        if (k < K) {
          const int q = 64 * k + lane;
          const bool pair = q >= qo0 && q < pair_end;
          const float2 nb = U.pxy[q + 1];
          if (pair && !polar_less(x[k], y[k], nb.x, nb.y)) {really = true;}
        }
      }
      if (__ballot(really) != 0ull) {return (uint32_t)(second_pass ? kDeferOther : kDeferOrder);}
    }
    if (zero_pair != 0ull) {return (uint32_t)kDeferOther;}
    put_words(U, kBitLK, vlk, lane);
    if (LFX_STAGE_ON(256u)) {
      put_words(U, kBitJL, vjl, lane);
      put_words(U, kBitJR, vjr, lane);
    }
  }
  LFX_STAMP(4);
  // ROWS: for the two window stages (E and the order masks of F) a lane takes CH CONSECUTIVE positions, CH * lane + d,
  // instead of one position per chunk: the windows of its positions overlap, so it reads 2 PT + CH values where the chunk
  // form reads CH x (2 PT + 1) -- 15 against 55 LDS reads per stage.  (Lane stride CH doubles: conflict-free for odd CH.)
  // The first and the last lanes' windows reach outside the two slabs: into the bit arrays before r[], the pad behind c[]
  // (UnitLds) -- finite or not, what is computed from such a value belongs to a position within PT of either end of the
  // slab, outside every block (a block keeps PT + 1 positions away from both ends of the span), and is thrown away: the
  // curvature is written as 0 there and the order mask of such a position meets an empty reach.  Round 5: the occlusion
  // fills, the reach and the pick rounds are in the rows form too (kRowPick; see row_frame above) and the labels come back
  // to the chunk form as ONE word per lane (two for the 12-chunk form).  For every compile-time PT a span of 3 .. 6 chunks
  // can hold, and for the long form of 12.
  constexpr bool kRows = PT > 0 && PT <= 2 * CH && (CH <= 6 || (CH == 12 && PT <= 5));     // (12 chunks: a window of 22 doubles per lane)
  constexpr bool kRowPick = kRows;
  constexpr int kRowWin = kRows ? 2 * PT + CH : 1;
  constexpr int kSetStride = CH < 4 ? 4 : CH;          // rows -> chunk form: the sets of a lane's word lie this far apart (final_label)
  const int p0 = CH * lane;
  // ---- D. occlusion fills (occlusion.hpp:37-91) and the reach of a pick inside the block (fill.hpp:101-117)
  uint32_t reach[CH];
  uint32_t rch[CH];                   // rows: reach of position p0 + d in the pick frame (bit PT + d = itself), 0 outside the block
  uint32_t occ_rows = 0, own_rows = 0;        // rows: bit d <-> position p0 + d is occluded / lies in the block
#pragma unroll
  for (int k = 0; k < (kRowPick ? 0 : CH); k++) {
    reach[k] = 0;
    if (k < K) {
      const int q = 64 * k + lane;
      const uint32_t lw = get_win(U, kBitLK, k, W0);
      int Lr = __clz((int)~(lw << 16));
      int Rr = __ffs((int)~(lw >> 16)) - 1;
      Lr = Lr < P ? Lr : P;
      Rr = Rr < P ? Rr : P;
      const uint32_t left = ((1u << (Lr + 1)) - 1u) << (15 - Lr);      // jumps at q-1 .. q-1-Lr reach q
      const uint32_t right = ((1u << (Rr + 1)) - 1u) << 16;            // jumps at q+1 .. q+1+Rr reach q
      if (LFX_STAGE_ON(256u)) {
        ovr[k / 10] |= ((get_win(U, kBitJL, k, W0) & left) | (get_win(U, kBitJR, k, W1) & right)) != 0u ? kOvrOccluded << (3 * (k % 10)) : 0u;
      }
      // inside the block the links are cut at its ends (label.hpp:157-159): clamp the runs
      const int Lb = Lr < q - qb0 ? Lr : q - qb0;
      const int Rb = Rr < qb1 - 1 - q ? Rr : qb1 - 1 - q;
      reach[k] = lanes(in_span(q, qb0, qb1)) ? (((1u << (Lb + Rb + 1)) - 1u) << (16 - Lb)) : 0u;
    }
  }
  LFX_WAVE_SYNC();        // the x / y slab is dead from here on: the curvature slab takes its place
  LFX_STAMP(5);
  // ---- E. curvature of the block's points (curvature.cpp:44-50); borders and halo stay 0 (by rows where kRows, see above)
  const int row_base = p0 - PT;
  if constexpr (kRows) {
    double w[kRowWin];
    lds_window_f64(&U.r[row_base], w);
#pragma unroll
    for (int d = 0; d < CH; d++) {
      double sum = 0.;                                                     // math.hpp:46-52: left to right from 0
#pragma unroll
      for (int t = 0; t <= 2 * PT; t++) {
        const double v = w[d + t];
        sum += (t == PT) ? v * (-2. * PT) : v;                             // r * 1.0 == r exactly
      }
      const int width = qb1 - qb0;
      U.c[p0 + d] = (uint32_t)(p0 + d - qb0) < (uint32_t)(width > 0 ? width : 0) ? sum * sum : 0.;
    }
  }
#pragma unroll
  for (int k = 0; k < (kRows ? 0 : CH); k++) {
    if (k < K) {
      const int q = 64 * k + lane;
      int qq = q < P ? P : q;                                            // keep the window inside the slab
      qq = qq > 64 * CH - 1 - P ? 64 * CH - 1 - P : qq;
      double sum = 0.;                                                   // math.hpp:46-52: left to right from 0
      if (PT > 0 && 2 * PT + 1 <= 11) {
        double w[2 * (PT > 0 ? PT : 0) + 1];
        lds_window_f64(&U.r[qq - PT], w);
#pragma unroll
        for (int d = -(PT > 0 ? PT : 0); d <= (PT > 0 ? PT : 0); d++) {
          const double v = w[d + PT];
          sum += (d == 0) ? v * (-2. * PT) : v;                          // r * 1.0 == r exactly
        }
      } else {
        for (int d = -P; d <= P; d++) {
          const double v = U.r[qq + d];
          sum += (d == 0) ? v * (-2. * P) : v;
        }
      }
      U.c[q] = lanes(in_span(q, qb0, qb1)) ? sum * sum : 0.;
    }
  }
  LFX_WAVE_SYNC();
  LFX_STAMP(6);
  // ---- F. block labelling (label.hpp:61-139): edge pass, then surface pass over what is still Default
  // lt: the order masks, and on top of them the position's candidacy where the curvature is in a register: bit 31
  // c >= edge threshold (label.hpp:80-82), bit 30 c <= surface threshold (label.hpp:119-121)
  // (a run-time P may need every bit for the order: the candidates then are wave masks of their own)
  asm volatile ("" ::: "memory");
  const double edge_thr = DEF ? 0.05 : tab->prm.edge_thr, surf_thr = DEF ? 0.05 : tab->prm.surf_thr;
  uint32_t lt[CH];
  uint64_t ecand[CH], scand[CH];
  constexpr uint32_t kEdgeCand = 1u << ((PT > 0 ? PT : 1) + 18), kSurfCand = 1u << ((PT > 0 ? PT : 1) + 17);     // (just above the order bits)
  if constexpr (kRowPick) {
    // rows all the way: lt[d] = the order mask of position p0 + d in the pick frame (bit PT + d + t <-> its neighbour at
    // offset t; the position's own bit 0), the candidates as bits of two words
    // (lanes 0 and 63, whose window was moved: every position of theirs lies outside the block, so their reach is 0 and
    // with it everything these masks are met with)
    constexpr int PR = PT > 0 ? PT : 1;
    double w[kRowWin];
    lds_window_f64(&U.c[row_base], w);
    uint32_t ec = 0, sc = 0;
#pragma unroll
    for (int d = 0; d < CH; d++) {
      const double ci = w[d + PR];
      uint32_t m = 0;
#pragma unroll
      for (int t = PR; t >= 1; t--) {m = m + m + (uint32_t)(w[d + PR + t] < ci);}
      m = m + m;
#pragma unroll
      for (int t = 1; t <= PR; t++) {m = m + m + (uint32_t)(w[d + PR - t] <= ci);}
      lt[d] = m << d;
      ec |= (ci >= edge_thr ? 1u : 0u) << d;                   // label.hpp:80-82
      sc |= (ci <= surf_thr ? 1u : 0u) << d;                   // label.hpp:119-121
    }
    // ---- D by rows (here rather than ahead of stage E: the reach masks are not live while the two windows are)
    {
      constexpr int kFrame = CH + 2 * PR;
      // link and jump windows: bit i <-> position p0 - PT - 1 + i (position p0 + d at PT + 1 + d)
      const uint32_t LW = get_win_at(U, kBitLK, p0 - PR - 1);
      uint32_t JLW = 0, JRW = 0;
      if (LFX_STAGE_ON(256u)) {
        JLW = get_win_at(U, kBitJL, p0 - PR - 1);
        JRW = get_win_at(U, kBitJR, p0 - PR - 1);
      }
      const uint32_t NL = ~LW, RNL = __builtin_bitreverse32(NL);
      // the block in the pick frame (bit i <-> position p0 - PT + i); the links are cut at its ends (label.hpp:157-159), which
      // for runs that start at a position of the block is the same as meeting them with the block
      int lo = qb0 - p0 + PR, hi = qb1 - p0 + PR;
      lo = lo < 0 ? 0 : (lo > kFrame ? kFrame : lo);
      hi = hi < 0 ? 0 : (hi > kFrame ? kFrame : hi);
      const uint32_t IB = hi > lo ? (((1u << (hi - lo)) - 1u) << lo) : 0u;
      own_rows = (IB >> PR) & ((1u << CH) - 1u);
#pragma unroll
      for (int d = 0; d < CH; d++) {
        const int fj = PR + 1 + d, fp = PR + d;
        // links at p - 1, p - 2, ... and at p, p + 1, ...: runs of at most PT (the stop bit), counted from the top
        const uint32_t Lr = (uint32_t)__builtin_clz((NL << (32 - fj)) | (1u << (31 - PR)));
        const uint32_t Rr = (uint32_t)__builtin_clz((RNL << fj) | (1u << (31 - PR)));
        // jumps at p - 1 .. p - 1 - Lr (far side to the right) and at p + 1 .. p + 1 + Rr (far side to the left) reach p
        const uint32_t o = ((JLW << (32 - fj)) >> (31u - Lr)) | ((JRW >> (fj + 1)) << (31u - Rr));
        occ_rows |= (o < 1u ? o : 1u) << d;
        const uint32_t run = (((1u << (Lr + Rr + 1u)) - 1u) << ((uint32_t)fp - Lr)) & IB;
        rch[d] = ((IB >> fp) & 1u) != 0u ? run : 0u;
      }
    }
    LFX_STAMP(7);
    // The pick rounds (label.hpp:72-95,113-134 / fill.hpp:101-117 as a priority fix-point): a live candidate with no live
    // candidate of higher priority in reach is picked; everything a pick reaches (the pick included) leaves the live set.
    uint32_t hp[CH];
    auto pick_pass = [&](uint32_t live) -> uint32_t {
      uint32_t sel = 0;
      for (;; ) {
        const uint32_t pk = live & ~row_hits<CH>(row_frame<CH, PR>(live), hp);
        // With a total order the live candidate of highest priority is always picked.  No pick at all means there is no
        // candidate left -- or the order is inconsistent (NaN curvature from non-finite input): stop instead of spinning.
        if (__builtin_amdgcn_ballot_w64(pk != 0u) == 0ull) {break;}
        sel |= pk;
        live &= ~row_hits<CH>(row_frame<CH, PR>(pk), rch);
        if (__builtin_amdgcn_ballot_w64(live != 0u) == 0ull) {break;}
      }
      return sel;
    };
    uint32_t sel_e = 0, sel_s = 0, by_e = 0, by_s = 0;         // picks; positions an edge / a surface pick reaches
    if (LFX_STAGE_KEPT(1u)) {
#pragma unroll
      for (int d = 0; d < CH; d++) {hp[d] = ~lt[d] & rch[d] & ~(1u << (PR + d));}      // edges: the higher curvature first
      sel_e = pick_pass(ec & own_rows);
      by_e = row_hits<CH>(row_frame<CH, PR>(sel_e), rch);
    }
    LFX_STAMP(8);
    if (LFX_STAGE_KEPT(64u)) {
#pragma unroll
      for (int d = 0; d < CH; d++) {hp[d] = lt[d] & rch[d];}                           // surfaces: the lower curvature first
      sel_s = pick_pass(sc & own_rows & ~by_e);                // in the block and still Default (label.hpp:119-121)
      by_s = row_hits<CH>(row_frame<CH, PR>(sel_s), rch);
    }
    // back to the chunk form: one word per lane through the range slab (dead since stage E), five sets of CH bits
    if constexpr (5 * kSetStride <= 32) {
      reinterpret_cast<u32_alias_t *>(U.r)[lane] =
        by_e | by_s << kSetStride | sel_s << (2 * kSetStride) | sel_e << (3 * kSetStride) | occ_rows << (4 * kSetStride);
    } else {
      // (the long form: five sets of twelve bits are sixty -- a pair of words per lane)
      static_assert(5 * kSetStride <= 64, "the five sets of a lane share two words");
      reinterpret_cast<u64_alias_t *>(U.r)[lane] = (uint64_t)by_e | (uint64_t)by_s << kSetStride | (uint64_t)sel_s << (2 * kSetStride) |
        (uint64_t)sel_e << (3 * kSetStride) | (uint64_t)occ_rows << (4 * kSetStride);
    }
    LFX_WAVE_SYNC();
  } else {
    // order masks, see order_masks(); the slab has no pad here: neighbours are read at clamped
    // positions, and what a clamped read yields is masked by `reach` (zero outside the block)
#pragma unroll
    for (int k = 0; k < CH; k++) {
      lt[k] = 0;
      ecand[k] = 0; scand[k] = 0;
      if (k < K) {
        const int q = 64 * k + lane;
        int qc = q < P ? P : q;
        qc = qc > span - 1 - P ? span - 1 - P : qc;
        uint32_t m = 0;
        if (PT > 0 && 2 * PT + 1 <= 11) {
          double w[2 * (PT > 0 ? PT : 0) + 1];
          lds_window_f64(&U.c[qc - PT], w);
          const double ci = w[PT];
          // bit 16 - d <-> c[q - d] <= c[q] (left neighbour: the lower index wins a tie), bit 16 + d <-> c[q + d] < c[q].
          // The bits are shifted in from the top one down, one compare and one add-with-carry each (m + m + bit): written
          // as a select of a bit constant per compare, the same mask cost a move, a select and an or per neighbour
#pragma unroll
          for (int d = (PT > 0 ? PT : 1); d >= 1; d--) {m = m + m + (uint32_t)(w[PT + d] < ci);}
          m = m + m;                                        // (bit 16, the position itself: nobody reads it)
#pragma unroll
          for (int d = 1; d <= (PT > 0 ? PT : 1); d++) {m = m + m + (uint32_t)(w[PT - d] <= ci);}
          m <<= 16 - (PT > 0 ? PT : 1);
          // (the slab is 0 outside the block, also where the window's centre was clamped, and the threshold is > 0)
          m |= ci >= edge_thr ? kEdgeCand : 0u;
          m |= ci <= surf_thr ? kSurfCand : 0u;
        } else {
          const double ci = U.c[qc];
          for (int d = 1; d <= P; d++) {
            const double cl = U.c[qc - d], cr = U.c[qc + d];
            m |= (cl <= ci) ? (1u << (16 - d)) : 0u;
            m |= (cr < ci) ? (1u << (16 + d)) : 0u;
          }
          ecand[k] = bal(ci >= edge_thr);
          scand[k] = bal(ci <= surf_thr);
        }
        lt[k] = m;
      }
    }
  }
  if constexpr (!kRowPick) {LFX_STAMP(7);}
#pragma unroll
  for (int pass = 0; pass < (kRowPick ? 0 : 2); pass++) {
    const bool edge = pass == 0;
    if (!edge) {LFX_STAMP(8);}
    if (!LFX_STAGE_KEPT(edge ? 1u : 64u)) {continue;}
    const int sel_arr = edge ? kBitSelE : kBitSelS;
    uint64_t A[CH], SEL[CH];
    uint32_t Hp[CH];
    uint64_t any = 0;
    WordVec va;                    // the live set as it stands in LDS
#pragma unroll
    for (int k = 0; k < CH; k++) {
      A[k] = 0; SEL[k] = 0; Hp[k] = 0;
      if (k < K) {
        const int q = 64 * k + lane;
        uint64_t cd;
        if (edge) {
          cd = PT > 0 ? bal((lt[k] & kEdgeCand) != 0u) : ecand[k];
        } else {
          // label.hpp:119-121: in the block and still Default, i.e. not reached by an edge pick
          const uint64_t low = PT > 0 ? bal((lt[k] & kSurfCand) != 0u) : scand[k];
          cd = in_span(q, qb0, qb1) & low & ~bal((get_win(U, kBitSelE, k, W0) & reach[k]) != 0u);
        }
        A[k] = cd;
        va.set(k, cd);
        any |= cd;
      }
    }
    if (any == 0ull) {continue;}
    put_words(U, kBitA, va, lane);
    // priority masks: which candidates in reach are visited first; bit 16 = the position itself
    // (reading the windows of all chunks ahead of the per-chunk work, so that the wave waits for LDS once per step of a
    // round rather than once per chunk, was measured and is slower: 1305 vs 1272 us, ten more registers live)
#pragma unroll
    for (int k = 0; k < CH; k++) {
      if (k < K && A[k] != 0ull) {
        const uint32_t m = get_win(U, kBitA, k, W0) & reach[k] & ~(1u << 16);
        Hp[k] = ((edge ? ~lt[k] : lt[k]) & m) | (1u << 16);
      }
    }
    // rounds: a live candidate with no live candidate of higher priority in reach is picked;
    // everything a pick reaches (the pick included) leaves the live set
    for (;; ) {
      uint64_t S[CH + 2];
      uint64_t picked = 0, left = 0;
      S[0] = 0; S[CH + 1] = 0;
      WordVec vs;
#pragma unroll
      for (int k = 0; k < CH; k++) {
        S[k + 1] = 0;
        if (k < K) {
          if (A[k] != 0ull) {
            S[k + 1] = bal((get_win(U, kBitA, k, W0) & Hp[k]) == (1u << 16));
            vs.set(k, S[k + 1]);
          }
          SEL[k] |= S[k + 1];
          picked |= S[k + 1];
        }
      }
      // With a total order the live candidate of highest priority is always picked.  No pick at all
      // means the order is inconsistent (NaN curvature from non-finite input): stop instead of spinning.
      if (picked == 0ull) {break;}
      put_words(U, kBitS, vs, lane);
#pragma unroll
      for (int k = 0; k < CH; k++) {
        if (k < K) {
          if ((S[k] | S[k + 1] | S[k + 2]) != 0ull) {
            A[k] &= ~bal((get_win(U, kBitS, k, W0) & reach[k]) != 0u);
            va.set(k, A[k]);
          }
          left |= A[k];
        }
      }
      if (left == 0ull) {break;}
      put_words(U, kBitA, va, lane);
    }
    {
      WordVec vsel;
#pragma unroll
      for (int k = 0; k < CH; k++) {
        if (k < K) {vsel.set(k, SEL[k]);}
      }
      put_words(U, sel_arr, vsel, lane);
    }
  }
  LFX_STAMP(9);
  // ---- G. final labels of the owned points (feature_extraction.cpp:133-138 order), outputs
  uint32_t pe = 0, ps = 0;
  asm volatile ("" ::: "memory");          // the table entries are not to be fetched (and held) any earlier
  uint8_t * __restrict__ label_s = tab->label_s;
  double * __restrict__ curv_s = tab->curv_s;
  // final label of position q = 64 k + lane (feature_extraction.cpp:133-138: the masks override the block labelling)
  auto final_label = [&](int k, int q) -> uint32_t {
    uint32_t l = kDefault;
    uint32_t t = (ovr[k / 10] >> (3 * (k % 10))) & 7u;
    if constexpr (kRowPick) {
      // position q is bit q mod CH of the five sets in the word of lane q / CH
      static_assert(row_div_exact<CH>(), "q / CH by multiplication");
      const uint32_t row = __umul24((uint32_t)q, RowDiv<CH>::kMul) >> RowDiv<CH>::kShift, d = (uint32_t)q - (uint32_t)CH * row;
      constexpr int S = kSetStride;
      uint32_t idx, occ_bit;
      if constexpr (5 * S > 32) {
        const uint64_t sets = reinterpret_cast<const u64_alias_t *>(U.r)[row] >> d;
        idx = ((uint32_t)sets & 1u) | ((uint32_t)(sets >> (S - 1)) & 2u) | ((uint32_t)(sets >> (2 * S - 2)) & 4u) | ((uint32_t)(sets >> (3 * S - 3)) & 8u);
        occ_bit = (uint32_t)(sets >> (4 * S)) & 1u;
      } else {
      const uint32_t sets = reinterpret_cast<const u32_alias_t *>(U.r)[row] >> d;
      // the four labelling bits side by side: reached by an edge pick | by a surface pick << 1 | surface pick << 2 | edge
      // pick << 3.  One multiplication moves bit i * S to bit 3 * (S - 1) + i (S = kSetStride): the partial product of bit
      // i * S with term 2^((3 - j)(S - 1)) lies at 3 (S - 1) + j + (i - j) S, which for i != j is outside the four bits
      // wanted when S >= 4, and the sixteen products are sixteen different powers of two (S and S - 1 are coprime, |j - j'|
      // < S), so nothing carries
      constexpr uint32_t kFour = 1u | 1u << S | 1u << (2 * S) | 1u << (3 * S);
      constexpr uint32_t kGather = 1u | 1u << (S - 1) | 1u << (2 * (S - 1)) | 1u << (3 * (S - 1));
      idx = (__umul24(sets & kFour, kGather) >> (3 * (S - 1))) & 15u;
      occ_bit = (sets >> (4 * S)) & 1u;
      }
      // EdgeNeighbor, then SurfaceNeighbor, then Surface, then Edge: the last one set wins (as the chunk form below)
      constexpr auto block_label = [](uint32_t i) -> uint64_t {
        return (i & 8u) ? kEdge : ((i & 4u) ? kSurface : ((i & 2u) ? kSurfaceNeighbor : ((i & 1u) ? kEdgeNeighbor : kDefault)));
      };
      constexpr uint64_t kBlockLabel =
        block_label(0) | block_label(1) << 4 | block_label(2) << 8 | block_label(3) << 12 | block_label(4) << 16 | block_label(5) << 20 |
        block_label(6) << 24 | block_label(7) << 28 | block_label(8) << 32 | block_label(9) << 36 | block_label(10) << 40 |
        block_label(11) << 44 | block_label(12) << 48 | block_label(13) << 52 | block_label(14) << 56 | block_label(15) << 60;
      l = (uint32_t)(kBlockLabel >> (4u * idx)) & 7u;
      t |= occ_bit;                                             // occluded (kOvrOccluded)
    } else {
      const uint32_t wE = get_win(U, kBitSelE, k, W0), wS = get_win(U, kBitSelS, k, W0);
      l = (wE & reach[k]) != 0u ? (uint32_t)kEdgeNeighbor : l;
      l = (wS & reach[k]) != 0u ? (uint32_t)kSurfaceNeighbor : l;
      l = (wS & (1u << 16)) != 0u ? (uint32_t)kSurface : l;
      l = (wE & (1u << 16)) != 0u ? (uint32_t)kEdge : l;
    }
    // occluded, then out of range, then parallel beam: the last one set wins -- a table of eight nibbles by the three bits
    constexpr uint32_t kOverride = (uint32_t)kOccluded << 4 | (uint32_t)kOutOfRange << 8 | (uint32_t)kOutOfRange << 12 |
      (uint32_t)kParallelBeam << 16 | (uint32_t)kParallelBeam << 20 | (uint32_t)kParallelBeam << 24 | (uint32_t)kParallelBeam << 28;
    l = t != 0u ? (kOverride >> (4u * t)) & 15u : l;
    return lanes(in_span(q, qo0, qo1)) ? l : (uint32_t)kDefault;
  };
  // The stores: a wave-uniform 64-bit part (table entry + the ring's start + the unit's first position, in scalar
  // registers) and a small unsigned lane part, through pointers declared global -- so that the store instructions take the
  // base from a scalar pair and a 32-bit offset per lane (a generic pointer with a signed 64-bit index made every store a
  // flat_ instruction behind a sign extension and three 64-bit adds per lane).  (off + g0 may lie a halo before the
  // ring's start: the lanes there own nothing and store nothing.)
  typedef __attribute__((address_space(1))) uint8_t g_u8_t;
  typedef __attribute__((address_space(1))) double g_f64_t;
  typedef __attribute__((address_space(1))) uint32_t g_u32_t;
  typedef float f32x4_t __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(1))) f32x4_t g_f32x4_t;
  g_u8_t * const label_u = (g_u8_t *)label_s + ((ptrdiff_t)off + g0);
  g_f64_t * const curv_u = (g_f64_t *)curv_s + ((ptrdiff_t)off + g0);
  g_f32x4_t * const rec_u = (g_f32x4_t *)tab->rec_pts + (off + rec_lo);
  g_u32_t * const idx_u = (g_u32_t *)tab->rec_idx + (off + rec_lo);
  g_u32_t * const sidx_u = SIDX ? (g_u32_t *)tab->sidx + ((ptrdiff_t)off + g0) : nullptr;      // (the holes form: where each position came from)
  (void)rec_hi;
  // The unit's feature records do not go out chunk by chunk into two arrays at the unit's place among the ring's
  // positions -- a handful of partial writes 4.8 KB away from the next unit's, which cost the kernel 150-180 us of its 1 020
  // (measured with the records ablated; tools/membench models it) -- but in rank order (edges, then surfaces) into the unit's
  // SLOT: up to kRecSlot points {x, y, z, c} and right behind them their indices, 20 kRecSlot bytes per unit, units back to back;
  // staged in the wave's LDS and written by one store per part.  A unit with more features than a slot holds puts the rest
  // at their ranks in the old arrays (feature_compact_kernel reads both).
  uint32_t lab[CH];
#pragma unroll
  for (int k = 0; k < CH; k++) {
    lab[k] = kDefault;
    if (k < K) {
      const int q = 64 * k + lane;
      const bool own = lanes(in_span(q, qo0, qo1));
      const uint32_t l = final_label(k, q);
      const double cv = U.c[q];
      if (own) {
        label_u[(uint32_t)q] = (uint8_t)l;
        if (curv_s != nullptr) {curv_u[(uint32_t)q] = cv;}       // (wave-uniform: a context created without LFX_OUT_CURVATURE has no such array)
#ifndef LFX_WHATIF_NO_SIDX       // (diagnostic: what the holes form's index array costs; downloads of such scans are wrong without it)
        if constexpr (SIDX) {sidx_u[(uint32_t)q] = src[k];}
#endif
      }
      const uint64_t fe = bal(l == kEdge), fs = bal(l == kSurface);
      lab[k] = l;
      pe += __popcll(fe);
      ps += __popcll(fs);
    }
  }
  {
    if ((pe | ps) != 0u && LFX_STAGE_ON(1024u)) {
      constexpr uint32_t kRecSlot = rec_slot_places(PT, CH);
      static_assert(kRecBytes * kRecSlot <= 8 * 64 * CH, "the range slab stages a slot's records");
      LFX_WAVE_SYNC();                               // (the range slab is dead since stage E; its words of the labelling have been read)
      f32x4_t * const stage_pts = reinterpret_cast<f32x4_t *>(U.r);
      u32_alias_t * const stage_idx = reinterpret_cast<u32_alias_t *>(stage_pts + kRecSlot);
      uint32_t re = 0, rs = pe;                      // ranks: the edges first, the surfaces behind them, each in position order
#pragma unroll
      for (int k = 0; k < CH; k++) {
        if (k < K) {
          const uint64_t fe = bal(lab[k] == kEdge), fs = bal(lab[k] == kSurface);
          if ((fe | fs) != 0ull) {
            if (lanes(fe | fs)) {
              const int q = 64 * k + lane, i = g0 + q;
              const uint32_t be = __builtin_amdgcn_mbcnt_hi((uint32_t)(fe >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)fe, 0u));
              const uint32_t bs = __builtin_amdgcn_mbcnt_hi((uint32_t)(fs >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)fs, 0u));
              const uint32_t rank = lab[k] == kEdge ? re + be : rs + bs;
              // AppendXYZIR (label.hpp:166-179): x, y, z and intensity <- (float)curvature; position i of ring `slot` is
              // point column * R + slot
              const f32x4_t rec = {x[k], y[k], z[k], (float)U.c[q]};
              const uint32_t idx = ORG ? (XF ? ring_column(og.xform[s * kRings + slot], (uint32_t)i, (uint32_t)N) : (uint32_t)i) * og.R + slot : src[k];
              if (rank < kRecSlot) {
                stage_pts[rank] = rec;
                stage_idx[rank] = idx;
              } else {
                rec_u[rank] = rec;                   // (more features than a slot holds: at their ranks among the unit's positions)
                idx_u[rank] = idx;
              }
            }
            re += (uint32_t)__popcll(fe);
            rs += (uint32_t)__popcll(fs);
          }
        }
      }
      LFX_WAVE_SYNC();
      const uint32_t staged = pe + ps < kRecSlot ? pe + ps : kRecSlot;
      g_f32x4_t * const slot_pts = (g_f32x4_t *)tab->rec32 + ((((size_t)s * max_rings + slot) * (uint32_t)B + (uint32_t)j) * (kRecSlot * kRecBytes / 16u));
      g_u32_t * const slot_idx = reinterpret_cast<g_u32_t *>(slot_pts + staged);      // (right behind the points that are there: one run of 20 bytes per record)
#pragma unroll
      for (uint32_t r0 = 0; r0 < kRecSlot; r0 += 64) {
        const uint32_t r = r0 + (uint32_t)lane;
        if (r < staged) {                            // one store of up to a kilobyte, one of up to 256 bytes
          slot_pts[r] = stage_pts[r];
          slot_idx[r] = stage_idx[r];
        }
      }
    }
  }
  LFX_STAMP(10);
  n_edge = pe;
  n_surface = ps;
  return 0u;
}

template<int PT, int CH, bool DEF, bool ORG, bool XF = false>
__device__ __forceinline__ void unit_body(
  const Params & prm, UnitLds<CH> * __restrict__ slabs, uint32_t ring_cap, uint32_t max_rings, uint32_t dbg_flags, uint32_t s,
  uint32_t slot, int j, const uint32_t * __restrict__ ring_count,
  const float2 * __restrict__ sxy, const float * __restrict__ sz,
  const uint32_t * __restrict__ sidx, const UnitTables * __restrict__ tab,
  uint32_t * __restrict__ defer_count, uint32_t * __restrict__ defer_list, bool second_pass, const OrgScan & og)
{
  const int lane = threadIdx.x & 63;
  UnitLds<CH> & U = slabs[ORG ? og.wave : 0u];
  const int P = PT > 0 ? PT : prm.P, B = prm.B;
  int N;
  int org_b0 = 0, org_b1 = 0;
  uint32_t scan_first = 0;                 // ORG: index of the scan's first point
  if (ORG) {
    // the scan must be R rings x C columns, C within the ring capacity (every unit of the scan sees the same: the host
    // has looked, and left the columns per ring and the block boundaries in the scan's row of `geom`)
    // (all four words are asked for before the first of them is tested: one round trip, not three)
    scan_first = og.scan_begin[s];
    const uint32_t C = og.geom[s * kGeomStride];
    org_b0 = (int)og.geom[s * kGeomStride + 1 + j];
    org_b1 = (int)og.geom[s * kGeomStride + 2 + j];
    // (the empty statement needs the values: left alone the compiler moves each load down to its first use, behind the
    // tests before it -- a memory round trip per test at the head of every wave)
    asm volatile ("" :: "s"(scan_first), "s"(C), "s"(org_b0), "s"(org_b1), "s"(ring_cap), "s"(B));
    N = (int)C;
    if (C == 0u) {
      if (og.r0 == 0u && j == 0 && og.wave == 0 && lane == 0) {scan_falls_back(tab, s);}
      return;
    }
  } else {
    N = (int)ring_count[s * kRings + slot];
    if (N == 0) {return;}                                  // no such ring in this scan
  }
  const size_t off = ring_base(s, slot, max_rings, ring_cap);
  // A deferred ring goes on `defer_list` once (the first unit to flag it appends it); the flag keeps
  // the reasons: kDeferOrder = not angle-sorted as bucketed (ring_order_kernel repairs that and the
  // ring gets a second pass here), kDeferOther = anything only the workgroup-per-ring kernel handles.
  // ORG: the whole scan goes to the bucketing route instead.
#define LFX_DEFER(reason) \
  do { \
    if (ORG) { \
      if (lane == 0) {scan_falls_back(tab, s, (reason) == kDeferOrder ? (uint32_t)kScanOrderFell : 0u);} \
    } else if (lane == 0 && (atomicOr(tab->ring_flags + s * kRings + slot, (reason)) & kDeferMask) == 0u) { \
      defer_list[atomicAdd(defer_count, 1u)] = s * kRings + slot; \
    } \
    return; \
  } while (0)
  LFX_STAMP(0);
  // skip conditions and over-long rings are the slow path's business (it also reports them); a ring longer than the
  // LDS-resident kernels take is the long-ring kernel's, whatever its blocks (the span word below packs positions in 15 bits)
  // (ORG: the same for the four waves of the workgroup, which therefore leave together -- before the barrier)
  if (N < 2 * P + 1 || N - 2 * P < B || (uint32_t)N > lds_ring_cap(ring_cap)) {
    if (j == 0) {LFX_DEFER(kDeferOther);}
    return;
  }
  int b0, b1;
  if (ORG) {
    b0 = org_b0;
    b1 = org_b1;
  } else {
    // both boundaries from one evaluation of the f64 formula: even lanes take j, odd lanes j + 1
    const int bj = block_boundary(N, P, B, j + (lane & 1));
    b0 = __builtin_amdgcn_readlane(bj, 0);
    b1 = __builtin_amdgcn_readlane(bj, 1);
  }
  const UnitGeom G = unit_geometry(N, P, B, j, b0, b1);
  if (b1 - b0 < 2 || G.span > (64 * CH)) {LFX_DEFER(kDeferOther);}
  const int o0 = G.o0, o1 = G.o1, g0 = G.g0, qlo = G.qlo, qhi = G.qhi;

  LFX_STAMP(1);
  // ---- A. load; x, y also to the wave's LDS slab (neighbours are read by position)
  {
    uint32_t * z = &U.bits[0][0];
    constexpr int kBitDwords = kUnitBitArrays * UnitLds<CH>::kBitWords;
#pragma unroll
    for (int w0 = 0; w0 < kBitDwords; w0 += 64) {
      if (w0 + 64 <= kBitDwords || lane + w0 < kBitDwords) {z[lane + w0] = 0u;}
    }
  }
  // z and the original index are only needed for the feature records at the very end; loaded here,
  // with x and y, their latency hides behind the whole computation instead of ending it (registers
  // are not what limits the waves per CU of this kernel, LDS is)
  float x[CH], y[CH], z[CH];
  uint32_t src[CH];
  if (ORG) {
    // lane = (column cq of a 16-column piece, ring `sub` of the group): four neighbouring lanes read the four
    // 32-byte records of one 128-byte line; wave w takes pieces w, w + 4, ... of the span
    const uint32_t sub = (uint32_t)lane & 3u, cq = (uint32_t)lane >> 2;
    const uint32_t rr = og.r0 + sub;
    const uint32_t rload = rr < og.R ? rr : og.R - 1u;          // a group beyond the last ring loads nothing new
    // Every loop of this stage runs over all CH chunks without a test of the span: the loads of every chunk are
    // issued before anything waits for one of them (with a branch per chunk the compiler waits for a chunk's ring
    // word before it issues the next chunk's loads: five memory round trips in a row at the head of every wave).
    // Positions beyond the span are clamped to the ring's last point and masked out like the halo outside the ring.
    float4 rec[CH];
    uint32_t rw[CH];
    const uint8_t * const base = og.pts + (size_t)scan_first * 32u;
    // XF: the rings of the stream arrive rotated (scan not cut at -pi) or reversed (clockwise sensor): position i of a
    // ring is column ring_column(xf, i, N), xf found per ring by ring_cut_kernel; the order check below still decides
    const uint32_t xf = XF ? og.xform[s * kRings + rload] : 0u;
#pragma unroll
    for (int m = 0; m < CH; m++) {
      const int q = 64 * m + 16 * (int)og.wave + (int)cq;
      int i = g0 + q;
      // (positions outside the span ask for the span's first / last record again: the same line as a neighbouring lane's,
      // where a ring point beyond the span would be a line nobody needs -- 3 % of the kernel's reads at 1800 columns)
      i = i < g0 + qlo ? g0 + qlo : (i > g0 + qhi - 1 ? g0 + qhi - 1 : i);
      const uint32_t col = XF ? ring_column(xf, (uint32_t)i, (uint32_t)N) : (uint32_t)i;
      const uint8_t * p = base + (col * og.R + rload) * 32u;                // a scan is < 2^27 points (host check)
      rec[m] = *reinterpret_cast<const float4 *>(p);
      rw[m] = *reinterpret_cast<const uint32_t *>(p + 20);
    }
    __builtin_amdgcn_sched_barrier(0);                // (the scheduler otherwise pulls the first chunk's ring test up between the loads)
    uint64_t wrong = 0;
    uint32_t zero_seen = 0;                           // (a (0, 0, 0) record among the unit's: the scan is one for the holes form)
    f32_alias_t * zex = reinterpret_cast<f32_alias_t *>(slabs[sub].r);
#pragma unroll
    for (int m = 0; m < CH; m++) {
      const int q = 64 * m + 16 * (int)og.wave + (int)cq;
      const uint64_t in = in_span(q, qlo, qhi);
      // the record must carry the ring id its place implies; with the zero-point filter on, a (0, 0, 0) record
      // would not be part of the scan (convert.py:162-163,192): not this kernel's case either
      uint64_t bad = bal((rw[m] & 0xFFFFu) != rr);
      if (og.drop_zero) {
        const uint64_t zb = bal(rec[m].x == 0.f) & bal(rec[m].y == 0.f) & bal(rec[m].z == 0.f);
        bad |= zb;
        zero_seen |= (zb & in) != 0ull ? 1u : 0u;
      }
      wrong |= bad & in;
      const bool inl = lanes(in);
      slabs[sub].pxy[q] = make_float2(inl ? rec[m].x : 0.f, inl ? rec[m].y : 0.f);
      zex[q] = rec[m].z;
    }
    wrong &= bal(rr < og.R);
    __syncthreads();                                  // the only workgroup barrier: the slabs are handed over
    if (wrong != 0ull) {
      if (zero_seen != 0u) {
        if (lane == 0) {scan_falls_back(tab, s, (uint32_t)kScanZeroFell);}
        return;
      }
      LFX_DEFER(kDeferOther);
    }
    if (slot >= og.R) {return;}                       // ring count not a multiple of four: no such ring
#pragma unroll
    for (int k = 0; k < CH; k++) {
      const int q = 64 * k + lane;
      const float2 v = U.pxy[q];
      x[k] = v.x; y[k] = v.y;
      z[k] = reinterpret_cast<const f32_alias_t *>(U.r)[q];
      src[k] = 0u;
    }
  } else {
    float2 v[CH];
#pragma unroll
    for (int k = 0; k < CH; k++) {                    // (all loads first, as above)
      const int q = 64 * k + lane;
      int i = g0 + q;
      i = i < 0 ? 0 : (i > N - 1 ? N - 1 : i);
      v[k] = sxy[off + i];
      z[k] = sz[off + i];
      src[k] = sidx[off + i];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < CH; k++) {
      const int q = 64 * k + lane;
      const bool in = lanes(in_span(q, qlo, qhi));
      x[k] = in ? v[k].x : 0.f;
      y[k] = in ? v[k].y : 0.f;
      U.pxy[q] = make_float2(x[k], y[k]);
    }
  }
  LFX_WAVE_SYNC();
  uint32_t pe = 0, ps = 0;
  {
    const uint32_t why = unit_core<PT, CH, DEF, ORG, XF>(prm, U, G, dbg_flags, s, slot, j, x, y, z, src, tab, second_pass, og, off, max_rings,
      (uint32_t)o0, (uint32_t)o1, pe, ps, lane);
    if (why != 0u) {LFX_DEFER(why);}
  }
  if (lane == 0) {
    const size_t ui = ((size_t)s * kRings + slot) * kUnitMaxBlocks + j;
    tab->unit_ne[ui] = pe;
    tab->unit_ns[ui] = ps;
    // owned positions [o0, o1) (N <= LFX_MAX_RING_POINTS < 32768); the top bit: this unit's records lie in its slot
    tab->unit_span[ui] = kUnitRecordsInSlot | ((uint32_t)o1 << 16) | (uint32_t)o0;
    if (ORG) {
      // the ring's totals, for the compaction (no kernel of their own on this route): two adds nobody waits for.  If the
      // scan falls back after all, the compaction takes the bucketing route's unit tables instead (feature_compact_kernel).
      (void)__hip_atomic_fetch_add(tab->ring_nedge + s * kRings + slot, pe, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      (void)__hip_atomic_fetch_add(tab->ring_nsurf + s * kRings + slot, ps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (j == 0) {
      tab->ring_status[s * kRings + slot] = kOk;
      if (ORG) {
        // what the bucketing kernel would have counted (it overwrites both if the scan falls back after all)
        og.ring_count_out[s * kRings + slot] = (uint32_t)N;
        if (slot == 0) {
          tab->scan_info[s * 4 + kInfoRings] = og.R;
          atomicOr(tab->scan_flags + s, (uint32_t)kScanFused);
        }
      }
    }
  }
#undef LFX_DEFER
}

// HOLES: the organised-scan form for a grid whose invalid returns are (0, 0, 0) records that the zero filter drops
// (lfx_config.drop_zero_points; convert.py:162-163,192).  Position k of ring r is then the ring's k-th VALID column: the
// ring's length, hence its block boundaries, and where in the grid a unit's positions lie all depend on the holes before
// them -- grid_count_kernel has left, per ring and piece of 16 columns, the number of valid returns before the piece (cum16).
// A workgroup is still block j of four adjacent rings, and its waves still load whole 128-byte lines, lane = (column of a
// piece, ring of the group): the first piece that holds a position one of the four units needs up to the last such piece
// (64 (CH + 2) columns at most: more holes than that and the scan is the bucketing route's).  Every wave works that range
// out for itself -- the four rows of the prefix table in registers, entry = lane, one round trip; geometry per lane for
// the ring of its records; start and end piece of each ring by ballot -- so that the hand-over through the slabs remains the
// workgroup's only barrier.  A valid record goes to slab position (prefix of its piece) + (its rank among the ring's valid
// records of the piece) - (the unit's first position); z and the record's COLUMN travel with it (the column is the
// position's original index: sidx, for the consumers).  From the hand-over on a unit is any other unit (unit_core).
template<int PT, int CH, bool DEF>
__device__ __forceinline__ void unit_body_holes(
  const Params & prm, UnitLds<CH> * __restrict__ slabs, uint32_t ring_cap, uint32_t max_rings, uint32_t dbg_flags, uint32_t s,
  uint32_t slot, int j, const UnitTables * __restrict__ tab, const OrgScan & og)
{
  constexpr int kLoads = holes_loads(CH);              // pieces a wave loads (4 waves: 4 kLoads pieces = 64 kLoads columns)
  constexpr int kQv = (kLoads + 3) / 4;                // registers that hold the prefixes of the workgroup's pieces, 16 per register and ring
  const int lane = threadIdx.x & 63;
  const uint32_t w = og.wave;
  UnitLds<CH> & U = slabs[w];
  const int P = PT > 0 ? PT : prm.P, B = prm.B;
  const uint32_t sub = (uint32_t)lane & 3u, cq = (uint32_t)lane >> 2;
  const uint32_t rr = og.r0 + sub, rload = rr < og.R ? rr : og.R - 1u;
  // ---- head: scalar loads only (one round trip through the scalar cache: the vector memory path is where the other waves'
  //      records queue -- with the four rows of the prefix table fetched and searched here a unit's head took 10 600 cycles of
  //      its 38 000, round 6) -- the scan's first point, its columns, its flags, and the four units' descriptors
  const uint32_t scan_first = og.scan_begin[s];
  const uint32_t C = og.geom[s * kGeomStride];
  const uint32_t flags = tab->scan_flags[s];
  const uint16_t * __restrict__ cum16 = tab->cum16;
  const uint4 * __restrict__ dsc = tab->hole_desc + ((size_t)s * og.R) * (uint32_t)B + (uint32_t)j;
  uint4 d[4];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const uint32_t ring = og.r0 + (uint32_t)r < og.R ? og.r0 + (uint32_t)r : og.R - 1u;
    d[r] = dsc[(size_t)ring * (uint32_t)B];
  }
  asm volatile ("" :: "s"(scan_first), "s"(C), "s"(flags), "s"(d[0].x), "s"(d[1].x), "s"(d[2].x), "s"(d[3].x));
  // (both tests are the same for the four waves: the count kernel set the bit before this kernel started)
  if (C == 0u || (flags & kScanCountFell) != 0u) {return;}
  const uint32_t stride = cum_stride(ring_cap);
  const int n_pieces = (int)((C + kPieceCols - 1u) / kPieceCols);
  LFX_STAMP(0);
  // ---- the pieces the four units need, and per lane the geometry of the unit its records belong to
  int pstart = 0x7FFFFFFF, pend = -1;
  int N_l = 0, b0_l = 0, b1_l = 0;
  bool dead_l = true;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const bool dead_r = og.r0 + (uint32_t)r >= og.R || ((d[r].y >> 16) & kHoleUnitDead) != 0u;
    if (!dead_r) {
      const int ps = (int)(d[r].z & 0xFFFFu), pe = (int)(d[r].z >> 16);
      pstart = ps < pstart ? ps : pstart;
      pend = pe > pend ? pe : pend;
    }
    if (sub == (uint32_t)r) {
      N_l = (int)(d[r].x & 0xFFFFu); b0_l = (int)(d[r].x >> 16); b1_l = (int)(d[r].y & 0xFFFFu);
      dead_l = dead_r;
    }
  }
  const int o0_l = j == 0 ? 0 : b0_l, o1_l = j == B - 1 ? N_l : b1_l;
  const int g0_l = o0_l - (P + 1);
  (void)o1_l;
  // this wave's own ring, as scalars (lane w holds ring r0 + w's values)
  const int N = __builtin_amdgcn_readlane(N_l, (int)w);
  const bool dead = __builtin_amdgcn_readlane((int)dead_l, (int)w) != 0;
  const int n_need = pend - pstart + 1;
  if (n_need <= 0 || n_need > 4 * kLoads) {return;}                    // none of the four rings has a unit here (more pieces than a workgroup loads: the count kernel has sent such a scan to the bucketing route)
  LFX_STAMP(13);
  uint32_t qv[kQv];
  {
    const uint16_t * row = cum16 + ((size_t)s * og.R + rload) * stride;
#pragma unroll
    for (int v = 0; v < kQv; v++) {
      const int e = pstart + 16 * v + (int)cq;
      qv[v] = row[e < n_pieces ? e : n_pieces];
    }
  }
  float4 rec[kLoads];
  const uint8_t * const base = og.pts + (size_t)scan_first * 32u + (size_t)rload * 32u;
#pragma unroll
  for (int m = 0; m < kLoads; m++) {
    const int t = 4 * m + (int)w;
    const uint32_t col = (uint32_t)(pstart + t) * kPieceCols + cq;
    rec[m] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < n_need && col < C) {rec[m] = *reinterpret_cast<const float4 *>(base + (size_t)col * og.R * 32u);}
  }
  {
    uint32_t * zb = &U.bits[0][0];
    constexpr int kBitDwords = kUnitBitArrays * UnitLds<CH>::kBitWords;
#pragma unroll
    for (int w0 = 0; w0 < kBitDwords; w0 += 64) {
      if (w0 + 64 <= kBitDwords || lane + w0 < kBitDwords) {zb[lane + w0] = 0u;}
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  // ---- the valid records to their positions in their ring's slab
  {
    f32_alias_t * zex = reinterpret_cast<f32_alias_t *>(slabs[sub].r);
    u32_alias_t * cex = reinterpret_cast<u32_alias_t *>(slabs[sub].r) + 64 * CH;      // (the columns: the upper half of the range slab)
    const uint64_t ring_lanes = 0x1111111111111111ull << sub;
#pragma unroll
    for (int m = 0; m < kLoads; m++) {
      const int t = 4 * m + (int)w;
      const uint32_t col = (uint32_t)(pstart + t) * kPieceCols + cq;
      const bool valid = t < n_need && col < C && !dead_l && !(rec[m].x == 0.f && rec[m].y == 0.f && rec[m].z == 0.f);
      const uint64_t vm = bal(valid) & ring_lanes;
      const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(vm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)vm, 0u));
      // the prefix of piece t of this lane's ring: held by lane 4 (t mod 16) + sub in register t / 16
      const uint32_t before = (uint32_t)__shfl((int)qv[(t >> 4) < kQv ? (t >> 4) : kQv - 1], 4 * (t & 15) + (int)sub);
      const int q = (int)(before + rank) - g0_l;
      if (valid && (uint32_t)q < (uint32_t)(64 * CH)) {
        slabs[sub].pxy[q] = make_float2(rec[m].x, rec[m].y);
        zex[q] = rec[m].z;
        cex[q] = col;
      }
    }
  }
  LFX_STAMP(14);
  __syncthreads();                                    // the only workgroup barrier: the slabs are handed over
  if (dead) {return;}
  const int b0 = __builtin_amdgcn_readlane(b0_l, (int)w), b1 = __builtin_amdgcn_readlane(b1_l, (int)w);
  const UnitGeom G = unit_geometry(N, P, B, j, b0, b1);
  const int o0 = G.o0, o1 = G.o1, qlo = G.qlo, qhi = G.qhi;
  const size_t off = ring_base(s, slot, max_rings, ring_cap);
  LFX_STAMP(1);
  float x[CH], y[CH], z[CH];
  uint32_t src[CH];
#pragma unroll
  for (int k = 0; k < CH; k++) {
    const int q = 64 * k + lane;
    const bool in = lanes(in_span(q, qlo, qhi));
    const float2 v = U.pxy[q];
    x[k] = in ? v.x : 0.f; y[k] = in ? v.y : 0.f;
    z[k] = reinterpret_cast<const f32_alias_t *>(U.r)[q];
    src[k] = reinterpret_cast<const u32_alias_t *>(U.r)[64 * CH + q] * og.R + slot;
  }
  LFX_WAVE_SYNC();
  // (positions outside the ring were never written: the slab's x, y there must read as zero for the window stages)
#pragma unroll
  for (int k = 0; k < CH; k++) {
    const int q = 64 * k + lane;
    if (!lanes(in_span(q, qlo, qhi))) {U.pxy[q] = make_float2(0.f, 0.f);}
  }
  LFX_WAVE_SYNC();
  uint32_t pe = 0, ps = 0;
  {
    const uint32_t why = unit_core<PT, CH, DEF, false, false, true>(prm, U, G, dbg_flags, s, slot, j, x, y, z, src, tab, false, og, off, max_rings,
      (uint32_t)o0, (uint32_t)o1, pe, ps, lane);
    if (why != 0u) {
      if (lane == 0) {scan_falls_back(tab, s, why == kDeferOrder ? (uint32_t)kScanOrderFell : 0u);}
      return;
    }
  }
  if (lane == 0) {
    const size_t ui = ((size_t)s * kRings + slot) * kUnitMaxBlocks + j;
    tab->unit_ne[ui] = pe;
    tab->unit_ns[ui] = ps;
    tab->unit_span[ui] = kUnitRecordsInSlot | ((uint32_t)o1 << 16) | (uint32_t)o0;
    (void)__hip_atomic_fetch_add(tab->ring_nedge + s * kRings + slot, pe, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_add(tab->ring_nsurf + s * kRings + slot, ps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // (the ring's length is in ring_count already, the scan's route bits in its flag word: grid_count_kernel; the number of
    // its rings that hold a point is counted by feature_compact_kernel)
    if (j == 0) {tab->ring_status[s * kRings + slot] = kOk;}
  }
}

// SECOND = false: first pass over the scans on the fall-back list (every scan of the batch when the organised-scan
// kernel is not in use), grid = (units of a scan / 4, list entries or fewer); rings it cannot take go on
// `defer_list` with the reason.  SECOND = true: second pass over the rings ring_order_kernel
// repaired (redo_list, grid-stride); what still cannot be taken goes on the slow list.
// V, the VARIANT of the parameters a kernel is compiled for (the host picks, lfx_api.hip): 0 = padding 5 and the reference's
// default thresholds as literals (hyper_parameter.hpp:35-43); 1 = padding 5, thresholds from the parameter block; 2 =
// padding 2 (the launch file's set, lidar_feature_extraction.param.yaml:3-10); 3 = any padding, at run time.  One
// unit_body per kernel: until round 5 the kernels for other than the default set carried three behind a run-time branch, and
// the register allocator budgeted for the worst of them (95-405 spilled scalar registers).
template<int V> struct UnitVariant
{
  static constexpr int kPT = V <= 1 ? 5 : (V == 2 ? 2 : 0);
  static constexpr bool kDEF = V == 0;
};

// (registers: the budget of the kernels that apply ring transforms -- at variant 0's 72 the 5-chunk forms spilled two vector
// registers to scratch; the LOOP forms, which keep a list walk's state live around the body, one workgroup per CU fewer again:
// they spilled 18-62.  Round 6: no kernel a stream can reach touches scratch, tools/kernel_resources.py.)
constexpr int unit_list_waves_per_simd(int ch, int variant, bool loop)
{
  // (variant 2 stages 128 records per unit from 5 chunks on: a workgroup per CU fewer there too)
  const int w = unit_waves_per_simd(ch, variant, true) - (variant == 2 && ch >= 5 ? 1 : 0);
  return loop ? (w > 4 ? (w - 3 < 4 ? w - 3 : 4) : (w > 1 ? w - 1 : 1)) : w;
}
template<int V, bool SECOND, int CH, bool LOOP = false>
__global__ __launch_bounds__(64 * kUnitWaves, unit_list_waves_per_simd(CH, V, LOOP)) void ring_unit_kernel(
  Params prm, uint32_t ring_cap, uint32_t dbg_flags, uint32_t max_rings, const uint32_t * __restrict__ ring_count,
  const float2 * __restrict__ sxy, const float * __restrict__ sz,
  const uint32_t * __restrict__ sidx, const UnitTables * __restrict__ tab,
  uint32_t * __restrict__ defer_count, uint32_t * __restrict__ defer_list,
  const uint32_t * __restrict__ redo_count, const uint32_t * __restrict__ redo_list, uint32_t redo_cap)
{
  constexpr int PT = UnitVariant<V>::kPT;
  constexpr bool DEF = UnitVariant<V>::kDEF;
  __shared__ UnitLds<CH> lds[kUnitWaves];
  // the wave index is the same in all 64 lanes: saying so keeps everything derived from it (unit,
  // ring length, block boundaries, chunk count) in scalar registers and its branches scalar
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  UnitLds<CH> * U = &lds[wave];
  const uint32_t B = (uint32_t)prm.B;
  uint32_t u = blockIdx.x * kUnitWaves + wave;
  const OrgScan none{nullptr, nullptr, nullptr, 0u, 0u, 0u, 0u, nullptr, nullptr};
  if (SECOND) {
    // one unit per wave here too: the grid covers every unit of the batch and the waves beyond the
    // repaired rings leave at once (a grid-stride loop around unit_body costs registers)
    const uint32_t n_redo = *redo_count < redo_cap ? *redo_count : redo_cap;      // the order kernel sent the rest to the slow list
    if (u >= n_redo * B) {return;}
    const uint32_t e = redo_list[u / B];
    const uint32_t s = e / kRings, slot = e % kRings;
    const int j = (int)(u % B);
    unit_body<PT, CH, DEF, false, false>(prm, U, ring_cap, max_rings, dbg_flags, s, slot, j, ring_count, sxy, sz, sidx, tab, defer_count,
      defer_list, true, none);
  } else {
    const uint32_t slot = u / B;
    if (slot >= max_rings) {return;}
    const int j = (int)(u % B);
    // (redo_count / redo_list double as the fall-back list here.)  LOOP = false: one list entry per blockIdx.y, the grid
    // covers the list (every scan of the batch is bucketed).  LOOP = true: the list is what the organised-scan kernel
    // gave up on, of a length the host can only guess, so a workgroup walks entries blockIdx.y, + gridDim.y, ...; the loop
    // around unit_body costs scalar registers, which is why the other form exists.
    const uint32_t n_list = *redo_count;
    for (uint32_t it = blockIdx.y; it < n_list; it += LOOP ? gridDim.y : n_list) {
      const uint32_t s = redo_list[it];
      unit_body<PT, CH, DEF, false, false>(prm, U, ring_cap, max_rings, dbg_flags, s, slot, j, ring_count, sxy, sz, sidx, tab, defer_count,
        defer_list, false, none);
      if (!LOOP) {break;}
      LFX_WAVE_SYNC();                       // the wave's slab is reused by the next entry
    }
  }
}

// The organised-scan kernel (unit_body<ORG>): workgroup = block j = blockIdx.y of four adjacent rings 4g .. 4g+3 of scan
// blockIdx.z, one ring per wave; which group g a workgroup takes follows from blockIdx.x and the scan (below).
// (Every scan on ONE XCD, so that the six units of a ring share an L2: measured, no difference -- profiles/r04_slices.
// An XCD taking FOUR adjacent groups of one scan, two scans sharing 32 workgroups: 1 061-1 064 against 1 052-1 054 us, round 5.)
#ifdef LFX_ORG_SGPRS       // (A/B: what the scalar-register budget of 8 workgroups per CU would cost this kernel)
#define LFX_ORG_ATTR __attribute__((amdgpu_num_sgpr(LFX_ORG_SGPRS)))
#else
#define LFX_ORG_ATTR
#endif
template<int V, int CH, bool XF, bool HOLES = false>
__global__ __launch_bounds__(64 * kUnitWaves, HOLES ? unit_list_waves_per_simd(CH, V, false) : unit_waves_per_simd(CH, V, XF)) LFX_ORG_ATTR void ring_unit_org_kernel(
  Params prm, uint32_t ring_cap, uint32_t dbg_flags, uint32_t max_rings, uint32_t drop_zero,
  const uint8_t * __restrict__ pts, const uint32_t * __restrict__ scan_begin, uint32_t * __restrict__ ring_count,
  const UnitTables * __restrict__ tab, const uint32_t * __restrict__ xform, const uint32_t * __restrict__ geom)
{
  static_assert(!(XF && HOLES), "the holes form takes rings as they stand");
  __shared__ UnitLds<CH> lds[kUnitWaves];
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // grid = (groups of four rings, blocks, scans): dispatched in the order group, block, scan, no division to find them.
  // Workgroups go to the eight XCDs round-robin by their linear index, i.e. by blockIdx.x mod 8 when the sensor has a
  // multiple of 32 rings -- and the records of ring group g are the 128-byte lines whose address bits 7-10 are g: taken
  // as they come, an XCD would only ever ask for ONE eighth of the address patterns (memory channels), and whatever makes
  // one of those slower holds up that XCD's whole share of the launch (round 5: stamps showed the waves of one XCD
  // waiting twice as long for their records as the others', its shader engines of the others idle for 17 % of the kernel).
  // So the ring group is turned by the scan index: every XCD sees every group.
  const int j = (int)blockIdx.y;
  const uint32_t s = blockIdx.z;
  uint32_t g = blockIdx.x;
#ifndef LFX_NO_GROUP_TURN
  {
    // (and with sixteen groups or a multiple an XCD takes two ADJACENT groups, 256 contiguous bytes of every column, at a
    // time: -2 % on the kernel, same box)
    const uint32_t groups = gridDim.x;
    const bool pairs = (groups & 15u) == 0u;
    if (pairs) {g = (g & ~15u) | ((g & 7u) << 1) | ((g >> 3) & 1u);}
    // (by two where the XCDs take pairs, so that a pair stays a pair; by one for the sensors of fewer rings, whose XCDs would
    // otherwise see every other group only)
    const uint32_t turn = (pairs ? 2u * s : s) & ((1u << (31 - __builtin_clz(groups))) - 1u);       // < groups
    g += turn;
    g = g >= groups ? g - groups : g;
  }
#endif
  const OrgScan og{pts, scan_begin, ring_count, max_rings, 4u * g, wave, drop_zero, xform, geom};
  const uint32_t slot = 4u * g + wave;
  if constexpr (HOLES) {
    unit_body_holes<UnitVariant<V>::kPT, CH, UnitVariant<V>::kDEF>(prm, lds, ring_cap, max_rings, dbg_flags, s, slot, j, tab, og);
    return;
  }
  unit_body<UnitVariant<V>::kPT, CH, UnitVariant<V>::kDEF, true, XF>(prm, lds, ring_cap, max_rings, dbg_flags, s, slot, j, nullptr, nullptr, nullptr, nullptr, tab, nullptr,
    nullptr, false, og);
}

// (The streaming form of this kernel -- waves walking their ring with the next unit's records arriving by LDS-DMA -- was
// built, measured slower and taken out again: git show 1488a09:lidar_feature_extraction_amd/csrc/lfx_kernels_extract.hpp,
// ring_stream_kernel; DESIGN.md 4 "Round 3".)


}  // namespace lfx
