// 3-D convex hull by quickhull, float64 throughout: the device passes of hull_topology.hpp (which states the algorithm, the
// degeneracy policy and why a call synchronises once per round and cannot be captured into a graph).
//   hull_farthest: the argmax of a metric, reduced in a fixed order -- each thread over its grid-stride elements, a tree per
//                  workgroup, then one workgroup over the partials (hull_final) -- with ties to the smallest point index, so the
//                  answer does not depend on the order of the live list.  No float atomics.
//   hull_mark / hull_assign: the faces a round replaces are flagged, the inserted point leaves, and the live points of flagged
//                  faces move to the new face that sees them from farthest or die.
//   hull_check:    every point against every face that is not flagged: the measured containment, and the re-homing the sweep of
//                  hull_run continues from.
//   hull_compact:  the live list without dead entries, through an integer cursor (the list's order is immaterial, see above).
// Compiled with -ffp-contract=off (Makefile): n . x + d is ((n0 x + n1 y) + n2 z) + d here, in hull_topology.hpp's hull_eval and
// in meshing.inside_planes, so a point the hull calls inside is inside for the cleaning that consumes the planes.
#include "common.hpp"
#include "dev_reduce.hpp"
#include "hull_topology.hpp"

namespace dns {

namespace {

constexpr int HL_BLOCK = 256;
constexpr int HL_PARTIALS = 1024;

struct HlPartial {
  double value;
  int32_t index;
  int32_t pad;
  int64_t live;
};

struct HlParam {
  double p[8];
};

struct HlWs {
  int32_t* face;     // [N] the face a point is homed to, -1 = dead
  int32_t* ids;      // [N] live list
  int32_t* ids2;     // [N] compaction target
  double* best;      // [N] hull_check's largest n . x + d
  double* planes;    // [cap][4]
  uint32_t* deadf;   // [cap] face replaced
  int32_t* dead_ids; // [cap] upload buffer
  HlPartial* partial;
  HullPick* record;
  uint32_t* cursor;
};

// The parts of the workspace of N points and cap faces into *w; returns its bytes (ws NULL: the size only).
size_t hl_layout(void* ws, uint64_t N, uint64_t cap, HlWs* w) {
  WsCarve c(ws);
  w->face = c.take<int32_t>(N);
  w->ids = c.take<int32_t>(N);
  w->ids2 = c.take<int32_t>(N);
  w->best = c.take<double>(N);
  w->planes = c.take<double>(cap * 4);
  w->deadf = c.take<uint32_t>(cap);
  w->dead_ids = c.take<int32_t>(cap);
  w->partial = c.take<HlPartial>(HL_PARTIALS);
  w->record = c.take<HullPick>(1);
  w->cursor = c.take<uint32_t>(64);                              // one word used; a whole 256-byte part
  return c.end();
}

__device__ __forceinline__ double hl_eval(const double* __restrict__ pl, double x, double y, double z) {
  return ((pl[0] * x + pl[1] * y) + pl[2] * z) + pl[3];
}

__device__ __forceinline__ bool hl_better(double va, int32_t ia, double vb, int32_t ib) {   // a beats b
  if (ia < 0) return false;
  if (ib < 0) return true;
  return va > vb || (va == vb && ia < ib);
}

// the workgroup's best (value, index) and its live count, valid in thread 0
__device__ __forceinline__ void hl_block_reduce(double& v, int32_t& i, int64_t& live) {
  __shared__ double sv[HL_BLOCK];
  __shared__ int32_t si[HL_BLOCK];
  __shared__ int64_t sl[HL_BLOCK];
  sv[threadIdx.x] = v, si[threadIdx.x] = i, sl[threadIdx.x] = live;
  __syncthreads();
  for (int s = HL_BLOCK / 2; s > 0; s >>= 1) {
    if (threadIdx.x < (uint32_t)s) {
      if (hl_better(sv[threadIdx.x + s], si[threadIdx.x + s], sv[threadIdx.x], si[threadIdx.x]))
        sv[threadIdx.x] = sv[threadIdx.x + s], si[threadIdx.x] = si[threadIdx.x + s];
      sl[threadIdx.x] += sl[threadIdx.x + s];
    }
    __syncthreads();
  }
  v = sv[0], i = si[0], live = sl[0];
}

__global__ __launch_bounds__(HL_BLOCK) void hull_farthest_kernel(int mode, HlParam prm, const double* __restrict__ pts, uint32_t n,
                                                                 const int32_t* __restrict__ ids, const int32_t* __restrict__ face,
                                                                 const double* __restrict__ planes, const double* __restrict__ best,
                                                                 HlPartial* __restrict__ partial) {
  double bv = 0.0;
  int32_t bi = -1;
  int64_t live = 0;
  for (uint64_t t = (uint64_t)blockIdx.x * HL_BLOCK + threadIdx.x; t < n; t += (uint64_t)gridDim.x * HL_BLOCK) {
    int32_t i = (int32_t)t;
    double val;
    if (mode == HULL_PICK_FACE) {
      i = ids[t];
      const int32_t f = face[i];
      if (f < 0) continue;
      val = hl_eval(planes + 4 * (size_t)f, pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]);
    } else if (mode == HULL_PICK_BEST) {
      val = best[i];
    } else {
      const double x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
      if (mode == HULL_PICK_LINE) {
        const double ax = x - prm.p[0], ay = y - prm.p[1], az = z - prm.p[2];
        const double cx = ay * prm.p[6] - az * prm.p[5], cy = az * prm.p[4] - ax * prm.p[6], cz = ax * prm.p[5] - ay * prm.p[4];
        val = (cx * cx + cy * cy) + cz * cz;
      } else {
        val = hl_eval(prm.p, x, y, z);
        if (mode == HULL_PICK_ABS) val = fabs(val);
      }
    }
    ++live;
    if (val == val && hl_better(val, i, bv, bi)) bv = val, bi = i;
  }
  hl_block_reduce(bv, bi, live);
  if (threadIdx.x == 0) partial[blockIdx.x] = HlPartial{bv, bi, 0, live};
}

__global__ __launch_bounds__(HL_BLOCK) void hull_final_kernel(const HlPartial* __restrict__ partial, uint32_t nb,
                                                              const double* __restrict__ pts, const int32_t* __restrict__ face,
                                                              HullPick* __restrict__ record) {
  double bv = 0.0;
  int32_t bi = -1;
  int64_t live = 0;
  for (uint32_t t = threadIdx.x; t < nb; t += HL_BLOCK) {
    live += partial[t].live;
    if (hl_better(partial[t].value, partial[t].index, bv, bi)) bv = partial[t].value, bi = partial[t].index;
  }
  hl_block_reduce(bv, bi, live);
  if (threadIdx.x == 0) {
    HullPick r;
    r.value = bv, r.index = bi, r.live = live;
    r.face = bi >= 0 ? face[bi] : -1;
    for (int a = 0; a < 3; ++a) r.x[a] = bi >= 0 ? pts[3 * (size_t)bi + a] : 0.0;
    *record = r;
  }
}

__global__ __launch_bounds__(HL_BLOCK) void hull_mark_kernel(const int32_t* __restrict__ dead_ids, uint32_t nd, uint32_t* __restrict__ deadf,
                                                             uint32_t first, uint32_t n_new, uint32_t cap, int32_t kill, uint32_t N,
                                                             int32_t* __restrict__ face) {
  const uint32_t t = blockIdx.x * HL_BLOCK + threadIdx.x;
  if (t < nd) {
    const uint32_t f = (uint32_t)dead_ids[t];
    if (f < cap) deadf[f] = 1u;
  }
  if (t < n_new && first + t < cap) deadf[first + t] = 0u;
  if (t == 0 && kill >= 0 && (uint32_t)kill < N) face[kill] = -1;
}

__global__ __launch_bounds__(HL_BLOCK) void hull_assign_kernel(const double* __restrict__ pts, const int32_t* __restrict__ ids, uint32_t n,
                                                               int32_t* __restrict__ face, const uint32_t* __restrict__ deadf,
                                                               const double* __restrict__ planes, uint32_t first, uint32_t n_new,
                                                               double see) {
  const uint64_t t = (uint64_t)blockIdx.x * HL_BLOCK + threadIdx.x;
  if (t >= n) return;
  const int32_t i = ids[t];
  const int32_t f = face[i];
  if (f < 0 || !deadf[f]) return;
  const double x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
  double bv = see;
  int32_t bf = -1;
  for (uint32_t j = 0; j < n_new; ++j) {
    const double v = hl_eval(planes + 4 * (size_t)(first + j), x, y, z);
    if (v > bv) bv = v, bf = (int32_t)(first + j);
  }
  face[i] = bf;
}

__global__ __launch_bounds__(HL_BLOCK) void hull_check_kernel(const double* __restrict__ pts, uint32_t N, const double* __restrict__ planes,
                                                              const uint32_t* __restrict__ deadf, uint32_t F, double see,
                                                              int32_t* __restrict__ face, int32_t* __restrict__ ids,
                                                              double* __restrict__ best) {
  const uint64_t i = (uint64_t)blockIdx.x * HL_BLOCK + threadIdx.x;
  if (i >= N) return;
  const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
  double bv = -INFINITY;
  int32_t bf = -1;
  for (uint32_t f = 0; f < F; ++f) {
    if (deadf[f]) continue;
    const double v = hl_eval(planes + 4 * (size_t)f, x, y, z);
    if (v > bv) bv = v, bf = (int32_t)f;
  }
  best[i] = bv;
  face[i] = bv > see ? bf : -1;
  ids[i] = (int32_t)i;
}

__global__ __launch_bounds__(HL_BLOCK) void hull_compact_kernel(const int32_t* __restrict__ ids, uint32_t n, const int32_t* __restrict__ face,
                                                                int32_t* __restrict__ ids2, uint32_t cap, uint32_t* __restrict__ cursor) {
  const uint64_t t = (uint64_t)blockIdx.x * HL_BLOCK + threadIdx.x;
  if (t >= n) return;
  const int32_t i = ids[t];
  if (face[i] < 0) return;
  const uint32_t at = atomicAdd(cursor, 1u);
  if (at < cap) ids2[at] = i;
}

struct HlBackend {
  const double* pts;
  uint32_t N, cap;
  double see;
  HlWs w;
  hipStream_t st;
  uint32_t n_list;
  bool failed = false;

  static dim3 blocks(uint64_t n) { return dim3((uint32_t)((n + HL_BLOCK - 1) / HL_BLOCK)); }
  bool ok(hipError_t e) {
    if (e != hipSuccess) {
      set_error("dns_convex_hull: %s", hipGetErrorString(e));
      failed = true;
    }
    return e == hipSuccess;
  }
  void set_see(double s) { see = s; }
  bool pick(int mode, const double* prm, HullPick& out) {
    HlParam p;
    for (int a = 0; a < 8; ++a) p.p[a] = prm[a];
    const uint32_t n = mode == HULL_PICK_FACE ? n_list : N;
    out.index = -1, out.live = 0, out.face = -1, out.value = 0.0;
    if (n == 0) return true;
    const uint32_t nb = std::min<uint64_t>(HL_PARTIALS, (n + (uint64_t)HL_BLOCK - 1) / HL_BLOCK);
    DNS_LAUNCH(hull_farthest_kernel, dim3(nb), dim3(HL_BLOCK), 0, st, mode, p, pts, n, (const int32_t*)w.ids, (const int32_t*)w.face,
               (const double*)w.planes, (const double*)w.best, w.partial);
    DNS_LAUNCH(hull_final_kernel, dim3(1), dim3(HL_BLOCK), 0, st, (const HlPartial*)w.partial, nb, pts, (const int32_t*)w.face, w.record);
    return ok(hipMemcpyAsync(&out, w.record, sizeof(HullPick), hipMemcpyDeviceToHost, st)) && ok(hipStreamSynchronize(st)) &&
           ok(hipGetLastError());
  }
  bool set_faces(int32_t first, int32_t n, const double* planes, const int32_t* dead, int32_t n_dead, int32_t kill) {
    if ((uint64_t)first + n > cap || (uint32_t)n_dead > cap) return false;
    if (!ok(hipMemcpyAsync(w.planes + 4 * (size_t)first, planes, (size_t)n * 32, hipMemcpyHostToDevice, st))) return false;
    if (n_dead && !ok(hipMemcpyAsync(w.dead_ids, dead, (size_t)n_dead * 4, hipMemcpyHostToDevice, st))) return false;
    DNS_LAUNCH(hull_mark_kernel, blocks(std::max(n, std::max(n_dead, 1))), dim3(HL_BLOCK), 0, st, (const int32_t*)w.dead_ids, (uint32_t)n_dead,
               w.deadf, (uint32_t)first, (uint32_t)n, cap, kill, N, w.face);
    // the host vectors behind `planes` and `dead` are rewritten next round: the copies above must have left them by then
    return ok(hipStreamSynchronize(st));
  }
  bool rehome(int32_t first, int32_t n) {
    if (n_list == 0) return true;
    DNS_LAUNCH(hull_assign_kernel, blocks(n_list), dim3(HL_BLOCK), 0, st, pts, (const int32_t*)w.ids, n_list, w.face, (const uint32_t*)w.deadf,
               (const double*)w.planes, (uint32_t)first, (uint32_t)n, see);
    return true;
  }
  bool check(int32_t n_faces) {
    DNS_LAUNCH(hull_check_kernel, blocks(N), dim3(HL_BLOCK), 0, st, pts, N, (const double*)w.planes, (const uint32_t*)w.deadf, (uint32_t)n_faces,
               see, w.face, w.ids, w.best);
    n_list = N;
    return true;
  }
  bool compact() {
    if (fill_words(w.cursor, 0u, 1, st, "dns_convex_hull") != DNS_OK) return false;
    DNS_LAUNCH(hull_compact_kernel, blocks(n_list), dim3(HL_BLOCK), 0, st, (const int32_t*)w.ids, n_list, (const int32_t*)w.face, w.ids2, N,
               w.cursor);
    uint32_t n = 0;
    if (!ok(hipMemcpyAsync(&n, w.cursor, 4, hipMemcpyDeviceToHost, st)) || !ok(hipStreamSynchronize(st))) return false;
    std::swap(w.ids, w.ids2);
    n_list = std::min(n, N);
    return true;
  }
};

}  // namespace

}  // namespace dns

using namespace dns;

extern "C" uint64_t dns_convex_hull_ws_bytes(uint32_t N, uint32_t face_cap) {
  if (N >= (1u << 31) || face_cap >= (1u << 28)) return 0;
  HlWs w;
  return hl_layout(nullptr, N, face_cap, &w);
}

extern "C" int dns_convex_hull(const double* points, uint32_t N, double eps, void* ws, uint32_t face_cap, int32_t* faces_out,
                               double* planes_out, uint32_t* n_faces_out, double* info, void* stream) {
  DNS_REQUIRE(N < (1u << 31) && face_cap >= 4 && face_cap < (1u << 28), "dns_convex_hull: N = %u (must be < 2^31), face_cap = %u (4 .. 2^28)", N,
              face_cap);
  DNS_REQUIRE(eps >= 0.0 && eps < INFINITY, "dns_convex_hull: eps must be finite and >= 0 (got %g)", eps);
  DNS_REQUIRE(N >= 4, "dns_convex_hull: points holds %u points; a hull in 3-D needs at least 4", N);
  DNS_REQUIRE(points && ws && faces_out && planes_out && n_faces_out && info, "dns_convex_hull: NULL argument");
  hipStream_t st = (hipStream_t)stream;
  int rc = ensure_ready(st, "dns_convex_hull");
  if (rc != DNS_OK) return rc;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) {
    set_error("dns_convex_hull: the stream is being captured; the hull synchronises every round and cannot be captured");
    return DNS_E_STATE;
  }
  HlBackend be;
  be.pts = points, be.N = N, be.cap = face_cap, be.st = st, be.n_list = 0;
  hl_layout(ws, N, face_cap, &be.w);
  be.see = eps;                                                // hull_run raises it to eps + tau once it knows the scale
  HullResult res;
  rc = fill_words(be.w.deadf, 0u, face_cap, st, "dns_convex_hull");
  if (rc != DNS_OK) return rc;
  const int code = hull_run(be, (int64_t)N, eps, (int32_t)face_cap, res);
  info[0] = res.max_outside, info[1] = (double)res.rounds, info[2] = (double)res.sweeps, info[3] = res.scale;
  *n_faces_out = 0;
  if (code == HULL_E_FACES) return 1;                            // the caller retries with a larger face_cap
  if (code == HULL_E_DEGENERATE) {
    set_error("dns_convex_hull: points are degenerate: all %u lie within eps of one plane (or line, or point)", N);
    return DNS_E_ARG;
  }
  if (code == HULL_E_BACKEND) {
    if (!be.failed) set_error("dns_convex_hull: a device pass was refused");
    return DNS_E_LAUNCH;
  }
  if (code != HULL_OK) {
    set_error("dns_convex_hull: the horizon of round %lld is not a single cycle, or %d sweeps did not settle the hull", (long long)res.rounds,
              HULL_MAX_SWEEPS);
    return DNS_E_STATE;
  }
  uint32_t nf = 0;
  for (const HullFace& f : res.faces) {
    if (f.dead) continue;
    for (int a = 0; a < 3; ++a) faces_out[3 * (size_t)nf + a] = f.v[a];
    for (int a = 0; a < 4; ++a) planes_out[4 * (size_t)nf + a] = f.pl[a];
    ++nf;
  }
  *n_faces_out = nf;
  return check_launch("dns_convex_hull");
}
