// lfx_kernels_deskew.hpp -- the sensor's motion during a sweep taken out of the two feature clouds (include/lfx.h, the de-skew
// section; no reference counterpart, LOAM's model).  One kernel body, the source of a record's firing time a template
// parameter; the arithmetic is the header's, in double, unfused.
#pragma once

#include "lfx_kernels_common.hpp"
#include "lfx_deskew_rows.hpp"

#pragma clang fp contract(off)

namespace lfx
{

// The constants of one scan's sweep are a row of doubles the host writes (lfx_deskew_rows.hpp).  A workgroup of the constant
// motion reads the row of blockIdx.y only: the addresses are the same for every lane, so the loads go through the scalar
// cache and the values live in scalar registers.
enum { kDskFromIndex = 0, kDskF32 = 1, kDskF64 = 2, kDskU32 = 3 };
enum { kTrjSegments = 64 };             // LDS columns per field (LFX_MAX_TRAJECTORY_KNOTS - 1 = 63 are used)
constexpr int kDeskewThreads = 256;

// what both kernels are told about the batch's records
struct DeskewRecords
{
  const uint32_t * scan_begin, * scan_info;
  const double * table;                 // [scans of the launch][kDskStride], or [segments of the launch][kTrjStride]
  const float4 * edge_in, * surf_in;    // (may be the outputs: in place)
  const uint32_t * edge_idx, * surf_idx;
  float4 * edge_out, * surf_out;
  const uint8_t * pts;                  // the batch's input records (a field source only)
  uint32_t step, off, be;
  uint32_t first;                       // the launch covers scans first .. first + gridDim.y - 1
};

struct DeskewArgs
{
  DeskewRecords rec;
  uint32_t to_end;
};

// The firing time of record idx of the scan of n records that starts at record b: idx / n, or the time field's value times
// `scale`.  NaN for an index that is no record of the scan: nothing is read, and the caller copies the record.
template<int SRC>
__device__ __forceinline__ double record_time(const DeskewRecords & A, size_t b, uint32_t idx, uint32_t n, double dn, double scale)
{
  if (SRC == kDskFromIndex) {return (double)idx / dn;}
  if (idx >= n) {return __builtin_nan("");}
  const uint8_t * f = A.pts + (b + idx) * A.step + A.off;
  double value;
  if (SRC == kDskF64) {
    uint64_t u = *reinterpret_cast<const uint64_t *>(f);
    if (A.be) {u = __builtin_bswap64(u);}
    value = __longlong_as_double((long long)u);
  } else {
    uint32_t u = *reinterpret_cast<const uint32_t *>(f);
    if (A.be) {u = __builtin_bswap32(u);}
    value = SRC == kDskF32 ? (double)__uint_as_float(u) : (double)u;
  }
  return value * scale;
}

// p rotated by the fraction f of the twist whose row row(field) reads (kRowK, kRowTheta, kRowW): w only in the small-angle
// form, k only in Rodrigues'.
template<typename Row>
__device__ __forceinline__ void rotate_by_fraction(Row row, double f, double px, double py, double pz, double & rx, double & ry, double & rz)
{
  const double theta = row(kRowTheta);
  if (theta < 1e-8) {
    const double wx = row(kRowW), wy = row(kRowW + 1), wz = row(kRowW + 2);
    rx = px + f * (wy * pz - wz * py);
    ry = py + f * (wz * px - wx * pz);
    rz = pz + f * (wx * py - wy * px);
  } else {
    const double kx = row(kRowK), ky = row(kRowK + 1), kz = row(kRowK + 2);
    const double a = f * theta, c = cos(a), sn = sin(a);
    const double cx = ky * pz - kz * py, cy = kz * px - kx * pz, cz = kx * py - ky * px;
    const double kdp = (kx * px + ky * py) + kz * pz, g = kdp * (1.0 - c);
    rx = (px * c + cx * sn) + kx * g;
    ry = (py * c + cy * sn) + ky * g;
    rz = (pz * c + cz * sn) + kz * g;
  }
}

// grid (chunks, scans) as feature_pack_kernel's; a grid-stride walk over the scan's n_edge + n_surface records, one float4
// load and one float4 store per record, its index from the list beside it.  No LDS, no atomics.
template<int SRC>
__global__ __launch_bounds__(kDeskewThreads) void deskew_kernel(const DeskewArgs args)
{
  const DeskewRecords & A = args.rec;
  const uint32_t s = A.first + blockIdx.y;
  const uint32_t ne = A.scan_info[s * 4 + kInfoEdge], ns = A.scan_info[s * 4 + kInfoSurface];
  const uint32_t b0 = A.scan_begin[s], n = A.scan_begin[s + 1] - b0;
  const size_t b = b0;
  const double * __restrict__ T = A.table + (size_t)blockIdx.y * kDskStride;
  // (all of the row is read here, ahead of the loop's stores, which the compiler must take to alias the table: scalar loads)
  const double twist[kRowW + 3] = {T[kRowK], T[kRowK + 1], T[kRowK + 2], T[kRowTheta], T[kRowW], T[kRowW + 1], T[kRowW + 2]};
  const double vx = T[kDskV], vy = T[kDskV + 1], vz = T[kDskV + 2];
  const double t0 = T[kDskT0], inv_dt = T[kDskInvDt], scale = T[kDskScale];
  const double r00 = T[kDskR + 0], r01 = T[kDskR + 1], r02 = T[kDskR + 2], r10 = T[kDskR + 3], r11 = T[kDskR + 4], r12 = T[kDskR + 5],
    r20 = T[kDskR + 6], r21 = T[kDskR + 7], r22 = T[kDskR + 8];
  const double dn = (double)n;
  for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < ne + ns; k += gridDim.x * blockDim.x) {
    const bool edge = k < ne;
    const uint32_t q = edge ? k : k - ne;
    const float4 rec = (edge ? A.edge_in : A.surf_in)[b + q];
    const uint32_t idx = (edge ? A.edge_idx : A.surf_idx)[b + q];
    const double t = record_time<SRC>(A, b, idx, n, dn, scale);
    const double alpha = SRC == kDskFromIndex ? t : (t - t0) * inv_dt;
    float4 out = rec;
    if (isfinite(alpha)) {
      double rx, ry, rz;                  // (the branch on theta is the same for every record of the scan)
      rotate_by_fraction([&](int f) {return twist[f];}, alpha, (double)rec.x, (double)rec.y, (double)rec.z, rx, ry, rz);
      const double mx = rx + alpha * vx, my = ry + alpha * vy, mz = rz + alpha * vz;
      if (args.to_end) {
        const double u0 = mx - vx, u1 = my - vy, u2 = mz - vz;
        out.x = (float)((r00 * u0 + r10 * u1) + r20 * u2);
        out.y = (float)((r01 * u0 + r11 * u1) + r21 * u2);
        out.z = (float)((r02 * u0 + r12 * u1) + r22 * u2);
      } else {
        out.x = (float)mx; out.y = (float)my; out.z = (float)mz;
      }
    }
    (edge ? A.edge_out : A.surf_out)[b + q] = out;
  }
}

// De-skew along a trajectory (include/lfx.h): the constants are a segment's, chosen per record by its time, so they cannot
// sit in scalar registers.
struct TrajectoryArgs
{
  const uint32_t * seg_begin;           // [scans of the launch + 1]: scan y's rows are seg_begin[y] .. seg_begin[y + 1] - 1
  DeskewRecords rec;
  double scale;                         // seconds per unit of the time field
};

// grid and walk as deskew_kernel's.  The scan's table is staged in LDS once per workgroup, ahead of the loop and of any
// store, FIELD-major [kTrjStride][kTrjSegments]: a 64-bit LDS read banks on (address / 4) mod 64 within 32 lanes, so lanes
// of one segment broadcast and lanes of different segments fall on different banks (a segment-major row of 192 bytes would
// put every segment on one of four offsets).  The segment comes from a fixed six-step search over the knot times in LDS
// whose predicate is exactly times[k] <= t.  No atomics.
template<int SRC>
__global__ __launch_bounds__(kDeskewThreads) void deskew_trajectory_kernel(const TrajectoryArgs args)
{
  const DeskewRecords & A = args.rec;
  __shared__ double seg[kTrjStride * kTrjSegments];
  const uint32_t s = A.first + blockIdx.y;
  const uint32_t ne = A.scan_info[s * 4 + kInfoEdge], ns = A.scan_info[s * 4 + kInfoSurface];
  if (blockIdx.x * blockDim.x >= ne + ns) {return;}      // (the whole workgroup: nothing to stage for)
  const uint32_t b0 = A.scan_begin[s], n = A.scan_begin[s + 1] - b0;
  const size_t b = b0;
  const uint32_t g0 = args.seg_begin[blockIdx.y];
  const uint32_t nseg = min(args.seg_begin[blockIdx.y + 1] - g0, (uint32_t)kTrjSegments - 1u);   // (the host refuses more)
  const double * __restrict__ T = A.table + (size_t)g0 * kTrjStride;
  for (uint32_t i = threadIdx.x; i < nseg * kTrjStride; i += blockDim.x) {
    const uint32_t j = i / kTrjStride, f = i - j * kTrjStride;
    seg[f * kTrjSegments + j] = T[i];
  }
  __syncthreads();
  const double * times = seg + kTrjTime * kTrjSegments;
  const double dn = (double)n;
  for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < ne + ns; k += gridDim.x * blockDim.x) {
    const bool edge = k < ne;
    const uint32_t q = edge ? k : k - ne;
    const float4 rec = (edge ? A.edge_in : A.surf_in)[b + q];
    const uint32_t idx = (edge ? A.edge_idx : A.surf_idx)[b + q];
    const double t = record_time<SRC>(A, b, idx, n, dn, args.scale);
    // knots with times[k] <= t among the segments' start times (the last knot never starts a segment); a NaN counts none
    uint32_t pos = 0;
#pragma unroll
    for (uint32_t step = kTrjSegments / 2; step; step >>= 1) {
      const uint32_t cand = pos + step;             // (at most 63: times[cand - 1] lies inside the array)
      const double tk = times[cand - 1];
      pos = ((cand <= nseg) & (tk <= t)) ? cand : pos;
    }
    const uint32_t j = (pos ? pos : 1u) - 1u;
    const double beta = (t - times[j]) * seg[kTrjInvDt * kTrjSegments + j];
    float4 out = rec;
    if (isfinite(beta)) {
      auto F = [&](int f) {return seg[f * kTrjSegments + j];};
      double rx, ry, rz;                  // (theta is the segment's: the lanes diverge in here)
      rotate_by_fraction(F, beta, (double)rec.x, (double)rec.y, (double)rec.z, rx, ry, rz);
      out.x = (float)(((F(kTrjA + 0) * rx + F(kTrjA + 1) * ry) + F(kTrjA + 2) * rz) + (F(kTrjQ + 0) + beta * F(kTrjDq + 0)));
      out.y = (float)(((F(kTrjA + 3) * rx + F(kTrjA + 4) * ry) + F(kTrjA + 5) * rz) + (F(kTrjQ + 1) + beta * F(kTrjDq + 1)));
      out.z = (float)(((F(kTrjA + 6) * rx + F(kTrjA + 7) * ry) + F(kTrjA + 8) * rz) + (F(kTrjQ + 2) + beta * F(kTrjDq + 2)));
    }
    (edge ? A.edge_out : A.surf_out)[b + q] = out;
  }
}

}  // namespace lfx
