// Host side of the 3-D convex hull (quickhull): the face/adjacency bookkeeping and the loop around three device passes.  HIP-free,
// on the precedent of scatter_plan.hpp: hull.hip drives it with kernels, tools/hull_topology_check.cpp with plain loops under the
// host sanitizers.
//
// The passes a backend supplies (all float64; face f SEES point x when n_f . x + d_f > see, see = eps + tau below):
//   pick(mode, prm)    the argmax of a metric over points, ties to the smallest point index, as a HullPick:
//                        HULL_PICK_FACE   live points: n . x + d of the point's own face (also returns the number of live points)
//                        HULL_PICK_PLANE  all points: prm[0..2] . x + prm[3]                    (simplex: min / max along x)
//                        HULL_PICK_LINE   all points: |(x - prm[0..2]) x prm[4..6]|^2           (simplex: farthest from a line)
//                        HULL_PICK_ABS    all points: |prm[0..2] . x + prm[3]|                  (simplex: farthest from a plane)
//                        HULL_PICK_BEST   all points: the value check() left per point          (the measured max_outside)
//   set_faces(first, n, planes, dead, n_dead, kill)   planes [n][4] of the new faces first .. first + n, the ids of the faces they
//                      replace, and the inserted point `kill` (it leaves the live list)
//   rehome(first, n)   every live point of a dead face moves to the new face that sees it from farthest (ties: the smaller face),
//                      or dies when none does
//   check(n_faces)     every point against every face that is not dead: its largest n . x + d is kept per point, the point is
//                      re-homed to that face when it is seen and dead otherwise, and the live list becomes all points again
//   set_see(see)       the threshold above, once the scale is known (before any set_faces)
//   compact()          the live list without its dead entries (called once fewer than an eighth of its entries are live)
// Every round ends in one pick whose record is read back (40 bytes: value, index, face, live count and the point's coordinates, so
// the host needs no copy of the points) and a stream synchronisation: hull_run is NOT graph-capturable.
//
// Degeneracy policy.  TSDF vertices lie on lattice edges, so exactly coplanar and collinear points are the normal case.  With
// L = the largest absolute coordinate and tau = 1e-12 L:
//   * a face sees a point only above eps + tau, so rounding noise on a face's own plane (hull vertices, duplicates of them, points
//     exactly coplanar with a finished face) never starts a round;
//   * when point p is inserted, the visible set is grown from p's own face over every neighbour g with n_g . p + d_g > -tau: a face
//     whose plane p lies on, or within tau below, is replaced as well.  Every horizon edge (a, b) then borders a face that p is
//     strictly below by more than tau, so p is not collinear with a and b and the new face (a, b, p) has a normal of non-zero
//     length (its area is at least |ab| tau / 2).  A normal that still fails to normalise is HULL_E_TOPOLOGY, never a returned face;
//   * the visible set is one connected region by construction; a horizon that is not a single cycle through distinct vertices
//     (possible only when rounding makes the visible region enclose a hidden face) is HULL_E_TOPOLOGY;
//   * replacing a face that p is up to tau below can uncover points by about tau, and a point of a replaced face is tested against
//     the new faces only.  So the result is not assumed: check() measures every point against every face, and while some point is
//     still seen the loop continues from it (at most HULL_MAX_SWEEPS times).  The value check() measured last is returned.
//   * fewer than four points, or all of them within eps + tau of one plane (or one line, or one point), is HULL_E_DEGENERATE.
#pragma once
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <array>
#include <unordered_map>
#include <vector>

namespace dns {

enum { HULL_PICK_FACE = 0, HULL_PICK_PLANE = 1, HULL_PICK_LINE = 2, HULL_PICK_ABS = 3, HULL_PICK_BEST = 4 };
enum { HULL_OK = 0, HULL_E_DEGENERATE = 1, HULL_E_FACES = 2, HULL_E_TOPOLOGY = 3, HULL_E_BACKEND = 4 };
constexpr int HULL_MAX_SWEEPS = 8;

struct HullPick {
  double value;
  int32_t index;   // -1: no point
  int32_t face;
  int64_t live;
  double x[3];
};

struct HullFace {
  int32_t v[3];
  int32_t adj[3];  // the face across edge v[k] -> v[(k + 1) % 3]
  double pl[4];
  bool dead;
};

struct HullResult {
  std::vector<HullFace> faces;       // every slot ever made; the hull is the faces that are not dead
  int64_t rounds = 0;
  int sweeps = 0;                    // check() passes made
  double max_outside = 0.0;
  double scale = 0.0;                // L
};

inline bool hull_plane(const double* a, const double* b, const double* c, double* pl) {
  const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
  const double vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
  double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
  const double len = sqrt(nx * nx + ny * ny + nz * nz);
  if (!(len > 0.0) || !std::isfinite(len)) return false;
  nx /= len, ny /= len, nz /= len;
  pl[0] = nx, pl[1] = ny, pl[2] = nz;
  pl[3] = -((nx * a[0] + ny * a[1]) + nz * a[2]);
  return true;
}

inline double hull_eval(const double* pl, const double* x) { return ((pl[0] * x[0] + pl[1] * x[1]) + pl[2] * x[2]) + pl[3]; }

// The whole loop.  `coords` collects the coordinates of every vertex the hull ever had (index -> xyz).
template <class Backend>
int hull_run(Backend& be, int64_t n_points, double eps, int32_t face_cap, HullResult& out) {
  if (n_points < 4) return HULL_E_DEGENERATE;
  std::unordered_map<int32_t, std::array<double, 3>> coords;
  auto remember = [&](const HullPick& p) { coords[p.index] = {p.x[0], p.x[1], p.x[2]}; };
  HullPick pk;
  double prm[8] = {0};
  // ---- scale and initial simplex: min / max along x, farthest from that line, farthest from that plane
  double L = 0.0;
  for (int a = 0; a < 3; ++a)
    for (int s = -1; s <= 1; s += 2) {
      double q[8] = {0};
      q[a] = (double)s;
      if (!be.pick(HULL_PICK_PLANE, q, pk)) return HULL_E_BACKEND;
      L = std::max(L, fabs(pk.value));
    }
  if (!std::isfinite(L)) return HULL_E_DEGENERATE;
  const double tau = 1e-12 * L, see = eps + tau;
  out.scale = L;
  be.set_see(see);
  HullPick s[4];
  prm[0] = -1.0;
  if (!be.pick(HULL_PICK_PLANE, prm, s[0])) return HULL_E_BACKEND;
  prm[0] = 1.0;
  if (!be.pick(HULL_PICK_PLANE, prm, s[1])) return HULL_E_BACKEND;
  double u[3] = {s[1].x[0] - s[0].x[0], s[1].x[1] - s[0].x[1], s[1].x[2] - s[0].x[2]};
  const double ul = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  if (s[0].index == s[1].index || !(ul > see)) {
    // no extent along x: any pair will do; take the extremes along y, then z
    bool found = false;
    for (int a = 1; a < 3 && !found; ++a) {
      double q[8] = {0};
      q[a] = -1.0;
      if (!be.pick(HULL_PICK_PLANE, q, s[0])) return HULL_E_BACKEND;
      q[a] = 1.0;
      if (!be.pick(HULL_PICK_PLANE, q, s[1])) return HULL_E_BACKEND;
      for (int c = 0; c < 3; ++c) u[c] = s[1].x[c] - s[0].x[c];
      found = s[0].index != s[1].index && sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) > see;
    }
    if (!found) return HULL_E_DEGENERATE;
  }
  const double ul2 = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  for (int c = 0; c < 3; ++c) prm[c] = s[0].x[c], prm[4 + c] = u[c] / ul2;
  if (!be.pick(HULL_PICK_LINE, prm, s[2])) return HULL_E_BACKEND;
  if (!(sqrt(s[2].value) > see)) return HULL_E_DEGENERATE;
  double pl[4];
  if (!hull_plane(s[0].x, s[1].x, s[2].x, pl)) return HULL_E_DEGENERATE;
  if (!be.pick(HULL_PICK_ABS, pl, s[3])) return HULL_E_BACKEND;
  if (!(s[3].value > see)) return HULL_E_DEGENERATE;
  for (int i = 0; i < 4; ++i) remember(s[i]);
  const double cen[3] = {(s[0].x[0] + s[1].x[0] + s[2].x[0] + s[3].x[0]) / 4, (s[0].x[1] + s[1].x[1] + s[2].x[1] + s[3].x[1]) / 4,
                         (s[0].x[2] + s[1].x[2] + s[2].x[2] + s[3].x[2]) / 4};
  std::vector<HullFace>& F = out.faces;
  F.clear();
  if (face_cap < 4) return HULL_E_FACES;
  static const int tri[4][3] = {{0, 1, 2}, {0, 3, 1}, {1, 3, 2}, {0, 2, 3}};
  for (int f = 0; f < 4; ++f) {
    HullFace h;
    int a = tri[f][0], b = tri[f][1], c = tri[f][2];
    if (!hull_plane(s[a].x, s[b].x, s[c].x, h.pl)) return HULL_E_DEGENERATE;
    if (hull_eval(h.pl, cen) > 0.0) {
      std::swap(b, c);
      if (!hull_plane(s[a].x, s[b].x, s[c].x, h.pl)) return HULL_E_DEGENERATE;
    }
    h.v[0] = s[a].index, h.v[1] = s[b].index, h.v[2] = s[c].index;
    h.adj[0] = h.adj[1] = h.adj[2] = -1;
    h.dead = false;
    F.push_back(h);
  }
  {
    std::unordered_map<uint64_t, int> edge;                       // directed edge -> 3 face + k
    for (int f = 0; f < 4; ++f)
      for (int k = 0; k < 3; ++k) edge[((uint64_t)(uint32_t)F[f].v[k] << 32) | (uint32_t)F[f].v[(k + 1) % 3]] = 3 * f + k;
    for (int f = 0; f < 4; ++f)
      for (int k = 0; k < 3; ++k) {
        auto it = edge.find(((uint64_t)(uint32_t)F[f].v[(k + 1) % 3] << 32) | (uint32_t)F[f].v[k]);
        if (it == edge.end()) return HULL_E_TOPOLOGY;
        F[f].adj[k] = it->second / 3;
      }
  }
  std::vector<double> planes;
  std::vector<int32_t> dead;
  for (int f = 0; f < 4; ++f) planes.insert(planes.end(), F[f].pl, F[f].pl + 4);
  if (!be.set_faces(0, 4, planes.data(), nullptr, 0, -1)) return HULL_E_BACKEND;

  std::vector<int32_t> stamp, stack, visible;
  std::vector<std::array<int32_t, 3>> horizon;                    // (a, b, hidden face); the visible face and its edge follow
  std::unordered_map<int32_t, int32_t> starts, ends;
  int32_t round_id = 0;
  int64_t alloc = n_points;
  for (out.sweeps = 0; out.sweeps < HULL_MAX_SWEEPS; ++out.sweeps) {
    if (!be.check((int32_t)F.size())) return HULL_E_BACKEND;
    alloc = n_points;
    if (!be.pick(HULL_PICK_BEST, prm, pk)) return HULL_E_BACKEND;
    out.max_outside = pk.value;
    bool first = true;
    while (true) {
      if (!be.pick(HULL_PICK_FACE, prm, pk)) return HULL_E_BACKEND;
      if (pk.index < 0 || pk.live == 0) break;
      first = false;
      if (pk.live * 8 < alloc) {
        if (!be.compact()) return HULL_E_BACKEND;
        alloc = pk.live;
      }
      if (pk.face < 0 || pk.face >= (int32_t)F.size() || F[pk.face].dead) return HULL_E_TOPOLOGY;
      ++out.rounds;
      remember(pk);
      // ---- the visible region, grown from the point's own face
      stamp.resize(F.size(), 0);
      ++round_id;
      visible.clear(), stack.clear(), horizon.clear();
      stack.push_back(pk.face);
      stamp[pk.face] = round_id;
      while (!stack.empty()) {
        const int32_t f = stack.back();
        stack.pop_back();
        visible.push_back(f);
        for (int k = 0; k < 3; ++k) {
          const int32_t g = F[f].adj[k];
          if (stamp[g] == round_id) continue;
          if (hull_eval(F[g].pl, pk.x) > -tau) {
            stamp[g] = round_id;
            stack.push_back(g);
          }
        }
      }
      for (int32_t f : visible)
        for (int k = 0; k < 3; ++k) {
          const int32_t g = F[f].adj[k];
          if (stamp[g] != round_id) horizon.push_back({F[f].v[k], F[f].v[(k + 1) % 3], g});
        }
      if (horizon.size() < 3) return HULL_E_TOPOLOGY;
      const int32_t first_new = (int32_t)F.size();
      const int32_t n_new = (int32_t)horizon.size();
      if ((int64_t)first_new + n_new > face_cap) return HULL_E_FACES;
      starts.clear(), ends.clear();
      for (int32_t i = 0; i < n_new; ++i) {
        if (!starts.emplace(horizon[i][0], first_new + i).second || !ends.emplace(horizon[i][1], first_new + i).second) return HULL_E_TOPOLOGY;
      }
      planes.clear();
      for (int32_t i = 0; i < n_new; ++i) {
        const int32_t a = horizon[i][0], b = horizon[i][1], g = horizon[i][2];
        HullFace h;
        h.v[0] = a, h.v[1] = b, h.v[2] = pk.index;
        if (!hull_plane(coords[a].data(), coords[b].data(), pk.x, h.pl)) return HULL_E_TOPOLOGY;
        auto nx = starts.find(b), pv = ends.find(a);
        if (nx == starts.end() || pv == ends.end()) return HULL_E_TOPOLOGY;
        h.adj[0] = g, h.adj[1] = nx->second, h.adj[2] = pv->second;
        h.dead = false;
        int k = 0;
        for (; k < 3; ++k)
          if (F[g].v[k] == b && F[g].v[(k + 1) % 3] == a) break;
        if (k == 3) return HULL_E_TOPOLOGY;
        F[g].adj[k] = first_new + i;
        planes.insert(planes.end(), h.pl, h.pl + 4);
        F.push_back(h);
      }
      dead.assign(visible.begin(), visible.end());
      for (int32_t f : visible) F[f].dead = true;
      if (!be.set_faces(first_new, n_new, planes.data(), dead.data(), (int32_t)dead.size(), pk.index)) return HULL_E_BACKEND;
      if (!be.rehome(first_new, n_new)) return HULL_E_BACKEND;
    }
    if (first) {                                                  // the sweep found no point that any face sees
      ++out.sweeps;
      return HULL_OK;
    }
  }
  return HULL_E_TOPOLOGY;
}

}  // namespace dns
