// Host check of the convex hull's topology code (dns_slam_amd/csrc/hull_topology.hpp) under the address and undefined-behaviour
// sanitizers.  No GPU is involved and nothing is loaded into Python: plain loops stand in for the device passes of csrc/hull.hip
// (same metrics, same tie rule, same evaluation order).  From the repository root:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -Wextra tools/hull_topology_check.cpp -o /tmp/hull_topology_check
//   /tmp/hull_topology_check
//
// Inputs: a 9^3 integer lattice (eps 0 and 1e-3), 2000 points on a sphere, a cube's corners plus its face centres, two coincident
// copies of a tetrahedron, and -- to be refused -- coplanar input and three points.  Each accepted result is held to the hull
// acceptance of tests/hull_ref.py, with r = 1e-9 L:
//   (a) the maximum of n . x + d over all points and faces, recomputed here, is <= eps + r and equals what hull_run reported;
//   (b) every point known to be a vertex of the true hull (the lattice's and cube's corners, every sphere point, the tetrahedron)
//       has max_f (n_f . v + d_f) >= -(eps + r);
//   (c) every directed edge has exactly one twin, normals are unit and finite, each face's own vertices lie within r of its plane,
//       and the mean of the hull's vertices is strictly inside.
#include <math.h>
#include <stdio.h>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>
#include "../dns_slam_amd/csrc/hull_topology.hpp"

using namespace dns;

static int g_fail = 0;
static std::string g_case;
#define CHECK(cond, ...)                                    \
  do {                                                      \
    if (!(cond)) {                                          \
      if (++g_fail <= 40) {                                 \
        printf("FAIL [%s] %s: ", g_case.c_str(), #cond);    \
        printf(__VA_ARGS__);                                \
        printf("\n");                                       \
      }                                                     \
    }                                                       \
  } while (0)

struct HostBackend {
  const std::vector<double>& pts;
  int64_t N;
  double see = 0.0;
  std::vector<int32_t> face, ids;
  std::vector<double> best, planes;
  std::vector<uint8_t> deadf;
  int64_t compactions = 0;

  explicit HostBackend(const std::vector<double>& p) : pts(p), N((int64_t)p.size() / 3), face(N, -1), best(N, 0.0) {}
  void set_see(double s) { see = s; }
  static bool better(double va, int32_t ia, double vb, int32_t ib) { return ia >= 0 && (ib < 0 || va > vb || (va == vb && ia < ib)); }
  bool pick(int mode, const double* prm, HullPick& out) {
    double bv = 0.0;
    int32_t bi = -1;
    int64_t live = 0;
    const int64_t n = mode == HULL_PICK_FACE ? (int64_t)ids.size() : N;
    for (int64_t t = 0; t < n; ++t) {
      int32_t i = (int32_t)t;
      double val;
      if (mode == HULL_PICK_FACE) {
        i = ids[t];
        if (face[i] < 0) continue;
        val = hull_eval(&planes[4 * (size_t)face[i]], &pts[3 * (size_t)i]);
      } else if (mode == HULL_PICK_BEST) {
        val = best[i];
      } else if (mode == HULL_PICK_LINE) {
        const double ax = pts[3 * i] - prm[0], ay = pts[3 * i + 1] - prm[1], az = pts[3 * i + 2] - prm[2];
        const double cx = ay * prm[6] - az * prm[5], cy = az * prm[4] - ax * prm[6], cz = ax * prm[5] - ay * prm[4];
        val = (cx * cx + cy * cy) + cz * cz;
      } else {
        val = hull_eval(prm, &pts[3 * (size_t)i]);
        if (mode == HULL_PICK_ABS) val = fabs(val);
      }
      ++live;
      if (val == val && better(val, i, bv, bi)) bv = val, bi = i;
    }
    out.value = bv, out.index = bi, out.live = live, out.face = bi >= 0 ? face[bi] : -1;
    for (int a = 0; a < 3; ++a) out.x[a] = bi >= 0 ? pts[3 * (size_t)bi + a] : 0.0;
    return true;
  }
  bool set_faces(int32_t first, int32_t n, const double* pl, const int32_t* dead, int32_t n_dead, int32_t kill) {
    if ((size_t)(first + n) > deadf.size()) deadf.resize(first + n, 0), planes.resize(4 * (size_t)(first + n));
    for (int32_t i = 0; i < 4 * n; ++i) planes[4 * (size_t)first + i] = pl[i];
    for (int32_t i = 0; i < n_dead; ++i) deadf.at(dead[i]) = 1;
    if (kill >= 0) face.at(kill) = -1;
    return true;
  }
  bool rehome(int32_t first, int32_t n) {
    for (int32_t i : ids) {
      const int32_t f = face[i];
      if (f < 0 || !deadf.at(f)) continue;
      double bv = see;
      int32_t bf = -1;
      for (int32_t j = 0; j < n; ++j) {
        const double v = hull_eval(&planes[4 * (size_t)(first + j)], &pts[3 * (size_t)i]);
        if (v > bv) bv = v, bf = first + j;
      }
      face[i] = bf;
    }
    return true;
  }
  bool check(int32_t n_faces) {
    ids.resize(N);
    for (int64_t i = 0; i < N; ++i) {
      double bv = -INFINITY;
      int32_t bf = -1;
      for (int32_t f = 0; f < n_faces; ++f) {
        if (deadf.at(f)) continue;
        const double v = hull_eval(&planes[4 * (size_t)f], &pts[3 * (size_t)i]);
        if (v > bv) bv = v, bf = f;
      }
      best[i] = bv, face[i] = bv > see ? bf : -1, ids[i] = (int32_t)i;
    }
    return true;
  }
  bool compact() {
    std::vector<int32_t> keep;
    for (int32_t i : ids)
      if (face[i] >= 0) keep.push_back(i);
    ids.swap(keep);
    ++compactions;
    return true;
  }
};

static void run_case(const char* name, const std::vector<double>& pts, double eps, const std::vector<int32_t>& extreme, int expect) {
  g_case = name;
  HostBackend be(pts);
  HullResult res;
  const int code = hull_run(be, be.N, eps, 1 << 20, res);
  printf("%-28s N %7lld eps %-7g -> code %d", name, (long long)be.N, eps, code);
  CHECK(code == expect, "code %d, expected %d", code, expect);
  if (code != HULL_OK || expect != HULL_OK) {
    printf("\n");
    return;
  }
  std::vector<const HullFace*> faces;
  for (const HullFace& f : res.faces)
    if (!f.dead) faces.push_back(&f);
  const double L = res.scale, r = 1e-9 * L;
  // (c) structure
  std::map<std::pair<int32_t, int32_t>, int> edges;
  std::set<int32_t> verts;
  for (const HullFace* f : faces) {
    const double nl = sqrt(f->pl[0] * f->pl[0] + f->pl[1] * f->pl[1] + f->pl[2] * f->pl[2]);
    CHECK(std::isfinite(nl) && fabs(nl - 1.0) < 1e-12 && std::isfinite(f->pl[3]), "normal length %g", nl);
    for (int k = 0; k < 3; ++k) {
      CHECK(f->v[k] >= 0 && f->v[k] < be.N, "vertex %d", f->v[k]);
      ++edges[{f->v[k], f->v[(k + 1) % 3]}];
      verts.insert(f->v[k]);
      const double d = hull_eval(f->pl, &pts[3 * (size_t)f->v[k]]);
      CHECK(fabs(d) <= r, "own vertex %g from its plane (r %g)", d, r);
      CHECK(f->adj[k] >= 0 && !res.faces[f->adj[k]].dead, "adjacency to a dead face");
    }
  }
  for (const auto& e : edges) {
    CHECK(e.second == 1, "directed edge %d->%d held %d times", e.first.first, e.first.second, e.second);
    CHECK(edges.count({e.first.second, e.first.first}) == 1, "edge %d->%d has no twin", e.first.first, e.first.second);
  }
  CHECK((int64_t)faces.size() == 2 * (int64_t)verts.size() - 4, "Euler: %zu faces, %zu vertices", faces.size(), verts.size());
  double mean[3] = {0, 0, 0};
  for (int32_t v : verts)
    for (int a = 0; a < 3; ++a) mean[a] += pts[3 * (size_t)v + a] / (double)verts.size();
  double mo = -INFINITY, deepest = -INFINITY;
  for (const HullFace* f : faces) {
    deepest = std::max(deepest, hull_eval(f->pl, mean));
    for (int64_t i = 0; i < be.N; ++i) mo = std::max(mo, hull_eval(f->pl, &pts[3 * (size_t)i]));
  }
  CHECK(deepest < 0.0, "the mean of the hull vertices is not strictly inside (%g)", deepest);
  // (a)
  CHECK(mo <= eps + r, "max_outside %g > eps + r = %g", mo, eps + r);
  CHECK(mo == res.max_outside, "max_outside recomputed %g, reported %g", mo, res.max_outside);
  // (b)
  for (int32_t v : extreme) {
    double m = -INFINITY;
    for (const HullFace* f : faces) m = std::max(m, hull_eval(f->pl, &pts[3 * (size_t)v]));
    CHECK(m >= -(eps + r), "extreme point %d lies %g inside", v, m);
  }
  printf(": %zu faces, %zu vertices, %lld rounds, %d sweeps, %lld compactions, max_outside %.3g\n", faces.size(), verts.size(),
         (long long)res.rounds, res.sweeps, (long long)be.compactions, mo);
}

int main() {
  std::mt19937_64 rng(7);
  std::normal_distribution<double> gauss(0.0, 1.0);
  {
    std::vector<double> p;
    std::vector<int32_t> corners;
    for (int x = 0; x < 9; ++x)
      for (int y = 0; y < 9; ++y)
        for (int z = 0; z < 9; ++z) {
          if ((x % 8 == 0) && (y % 8 == 0) && (z % 8 == 0)) corners.push_back((int32_t)p.size() / 3);
          p.push_back(x), p.push_back(y), p.push_back(z);
        }
    run_case("lattice 9^3", p, 0.0, corners, HULL_OK);
    run_case("lattice 9^3 eps 1e-3", p, 1e-3, corners, HULL_OK);
  }
  {
    std::vector<double> p;
    std::vector<int32_t> all;
    for (int i = 0; i < 2000; ++i) {
      double v[3] = {gauss(rng), gauss(rng), gauss(rng)};
      const double l = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
      for (int a = 0; a < 3; ++a) p.push_back(v[a] / l);
      all.push_back(i);
    }
    run_case("sphere 2000", p, 0.0, all, HULL_OK);
  }
  {
    std::vector<double> p;
    std::vector<int32_t> corners;
    for (int c = 0; c < 8; ++c) {
      corners.push_back(c);
      p.push_back(c & 1), p.push_back((c >> 1) & 1), p.push_back(c >> 2);
    }
    for (int a = 0; a < 3; ++a)
      for (int s = 0; s < 2; ++s) {
        double v[3] = {0.5, 0.5, 0.5};
        v[a] = s;
        p.insert(p.end(), v, v + 3);
      }
    run_case("cube + face centres", p, 0.0, corners, HULL_OK);
  }
  {
    const double t[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0.2, 0.3, 1};
    std::vector<double> p(t, t + 12);
    p.insert(p.end(), t, t + 12);
    run_case("tetrahedron twice", p, 0.0, {0, 1, 2, 3, 4, 5, 6, 7}, HULL_OK);
  }
  {
    std::vector<double> p;
    for (int x = 0; x < 6; ++x)
      for (int y = 0; y < 6; ++y) p.push_back(x), p.push_back(y), p.push_back(2.0 * x - y + 1.0);
    run_case("coplanar (refused)", p, 0.0, {}, HULL_E_DEGENERATE);
    std::vector<double> q(p.begin(), p.begin() + 9);
    run_case("three points (refused)", q, 0.0, {}, HULL_E_DEGENERATE);
  }
  printf(g_fail ? "FAILED: %d checks\n" : "ok\n", g_fail);
  return g_fail ? 1 : 0;
}
