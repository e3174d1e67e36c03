// tests/host/test_voxel_port.cpp — a-loam_amd/csrc/voxel_device.hpp (the cell arithmetic the four device filters share) compiled for the host and
// checked against pcl::VoxelGrid<PointXYZI>::filter of the oracle's PCL stand-in (oracle/ref_shim/include/shim/pcl_shim.hpp), bit for bit.
//
// A host filter is assembled from the header alone: box -> cell index -> std::sort of {idx, pt} entries compared on idx only (what the stand-in does, so
// this toolchain's std::sort leaves both index vectors in the same order) -> centroid accumulator.  Its output must equal the stand-in's in count and in
// every float on seeded clouds of 1 .. 400 points with leaves 0.2 / 0.4 / 0.8: a few metres across, +-200 m, +-4000 m (unfiltered), points exactly on cell
// borders of both signs with -0.0f, all points in one cell, two opposite corners at +-3e5 (unfiltered).
// Beside it, the two arguments that decide which path a segment takes on the device:
//   - wherever every point passes the pack's range test and the integer guard decides, the packed-cell box and index equal the float ones point for point;
//   - wherever all |floor(p * inv)| < 2^23, "cell differs from predecessor" equals "index differs from predecessor" for consecutive points (the index in
//     128 bits, so that the statement also covers boxes PCL does not filter; on filtered boxes it must be cell_index itself).
// Exit status 0 only when everything is equal and every branch was taken often enough.  Build: g++ -O2 -std=c++17 -ffp-contract=off.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <random>
#include <vector>

#include "shim/pcl_shim.hpp"
#include "../../a-loam_amd/csrc/voxel_device.hpp"

namespace vx = aloam::voxel;
typedef pcl::PointXYZI P;

static int g_failures = 0;
static void fail(int cloud, const char* what) {
  if (g_failures++ < 20) std::printf("cloud %d: %s\n", cloud, what);
}

// pcl::VoxelGrid::filter from voxel_device.hpp alone; *unfiltered as the header decides it
static std::vector<P> header_filter(const std::vector<P>& in, float leaf, bool* unfiltered) {
  const float inv = vx::inverse_leaf(leaf);
  float mn[3] = {3.402823466e38f, 3.402823466e38f, 3.402823466e38f}, mx[3] = {-3.402823466e38f, -3.402823466e38f, -3.402823466e38f};
  for (const P& p : in) {
    mn[0] = fminf(mn[0], p.x); mx[0] = fmaxf(mx[0], p.x);
    mn[1] = fminf(mn[1], p.y); mx[1] = fmaxf(mx[1], p.y);
    mn[2] = fminf(mn[2], p.z); mx[2] = fmaxf(mx[2], p.z);
  }
  const vx::Box box = vx::make_box(mn, mx, inv);
  *unfiltered = box.unfiltered;
  if (box.unfiltered) return in;
  struct Entry { unsigned idx; unsigned pt; bool operator<(const Entry& o) const { return idx < o.idx; } };
  std::vector<Entry> ev;
  ev.reserve(in.size());
  for (size_t i = 0; i < in.size(); ++i) ev.push_back(Entry{vx::cell_index(box, in[i].x, in[i].y, in[i].z, inv), (unsigned)i});
  std::sort(ev.begin(), ev.end(), std::less<Entry>());
  std::vector<P> out;
  for (size_t a = 0; a < ev.size();) {
    vx::Centroid c;
    size_t b = a;
    for (; b < ev.size() && ev[b].idx == ev[a].idx; ++b) { const P& p = in[ev[b].pt]; c.add(p.x, p.y, p.z, p.intensity); }
    P o;
    c.get(o.x, o.y, o.z, o.intensity);
    out.push_back(o);
    a = b;
  }
  return out;
}

int main() {
  std::mt19937 rng(20240607u);
  auto uni = [&](float lo, float hi) { return std::uniform_real_distribution<float>(lo, hi)(rng); };
  auto uint_in = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); };
  const float leaves[3] = {0.2f, 0.4f, 0.8f};
  const int kClouds = 3000;
  long long n_points = 0;
  int n_unfiltered = 0, n_decided = 0, n_border = 0, n_exact = 0;
  for (int c = 0; c < kClouds; ++c) {
    const int family = c % 6;
    const float leaf = leaves[(c / 6) % 3];
    const int n = c < 6 * 3 ? 1 : uint_in(1, 400);   // every family at every leaf once with a single point
    std::vector<P> pts(n);
    const float cx = uni(-30.f, 30.f), cy = uni(-30.f, 30.f), cz = uni(-3.f, 3.f);
    const int kb = uint_in(-40, 40);
    for (int i = 0; i < n; ++i) {
      P p;
      switch (family) {
        case 0: p.x = cx + uni(-3.f, 3.f); p.y = cy + uni(-3.f, 3.f); p.z = cz + uni(-1.f, 1.f); break;   // a few metres across
        case 1: p.x = uni(-200.f, 200.f); p.y = uni(-200.f, 200.f); p.z = uni(-200.f, 200.f); break;
        case 2: p.x = uni(-4000.f, 4000.f); p.y = uni(-4000.f, 4000.f); p.z = uni(-4000.f, 4000.f); break;
        case 3: {                                                                                       // exactly on cell borders, both signs, -0.0f
          const int kx = uint_in(-12, 12), ky = uint_in(-12, 12), kz = uint_in(-4, 4);
          p.x = (float)kx * leaf; p.y = (float)ky * leaf; p.z = (float)kz * leaf;
          if (kx == 0 && (i & 1)) p.x = -0.0f;
          if (ky == 0 && (i & 2)) p.y = -0.0f;
          if (kz == 0 && (i & 1)) p.z = -0.0f;
          if (i % 5 == 4) p.x += uni(-leaf, leaf);                                                      // and some points off the borders among them
          break;
        }
        case 4: p.x = ((float)kb + uni(0.05f, 0.95f)) * leaf; p.y = ((float)-kb + uni(0.05f, 0.95f)) * leaf; p.z = uni(0.05f, 0.95f) * leaf; break;   // one cell
        default:                                                                                        // two opposite corners at +-3e5
          if (i == 0 && n > 1) { p.x = p.y = p.z = -3.0e5f; }
          else if (i == n - 1) { p.x = p.y = p.z = 3.0e5f; }
          else { p.x = cx + uni(-3.f, 3.f); p.y = cy + uni(-3.f, 3.f); p.z = cz + uni(-1.f, 1.f); }
      }
      p.intensity = (float)uint_in(0, 63) + uni(0.f, 0.1f);                                             // ring + relative time, as the pipeline carries it
      pts[i] = p;
    }
    n_points += n;
    if (family == 3) ++n_border;

    // ---- the filter itself -----------------------------------------------------------------------------------------------------------------
    auto cloud = std::make_shared<pcl::PointCloud<P>>();
    cloud->points = pts;
    pcl::VoxelGrid<P> vg;
    vg.setInputCloud(cloud);
    vg.setLeafSize(leaf, leaf, leaf);
    pcl::PointCloud<P> ref;
    vg.filter(ref);
    bool unfiltered = false;
    const std::vector<P> got = header_filter(pts, leaf, &unfiltered);
    if (got.size() != ref.points.size()) { fail(c, "number of output points differs"); continue; }
    bool same = true;
    for (size_t i = 0; i < got.size(); ++i) {
      const float a[4] = {got[i].x, got[i].y, got[i].z, got[i].intensity}, b[4] = {ref.points[i].x, ref.points[i].y, ref.points[i].z, ref.points[i].intensity};
      if (std::memcmp(a, b, sizeof a) != 0) same = false;
    }
    if (!same) fail(c, "an output float differs");
    if (unfiltered) ++n_unfiltered;

    // ---- the box again, for the two path arguments ----------------------------------------------------------------------------------------------
    const float inv = vx::inverse_leaf(leaf);
    float mn[3] = {3.402823466e38f, 3.402823466e38f, 3.402823466e38f}, mx[3] = {-3.402823466e38f, -3.402823466e38f, -3.402823466e38f};
    for (const P& p : pts) {
      mn[0] = fminf(mn[0], p.x); mx[0] = fmaxf(mx[0], p.x);
      mn[1] = fminf(mn[1], p.y); mx[1] = fmaxf(mx[1], p.y);
      mn[2] = fminf(mn[2], p.z); mx[2] = fmaxf(mx[2], p.z);
    }
    const vx::Box box = vx::make_box(mn, mx, inv);
    bool packable = true, exact = true;
    for (const P& p : pts) {
      const float fx = vx::cell_coord(p.x, inv), fy = vx::cell_coord(p.y, inv), fz = vx::cell_coord(p.z, inv);
      packable = packable && vx::cell_packable(fx, fy, fz);
      exact = exact && vx::cell_exact(fx, fy, fz);
    }
    if (packable) {                                                           // packed cells: the integer path of k_ring_features
      std::vector<unsigned> cells(n);
      int imn[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, imx[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
      for (int i = 0; i < n; ++i) {
        cells[i] = vx::pack_cell(vx::cell_coord(pts[i].x, inv), vx::cell_coord(pts[i].y, inv), vx::cell_coord(pts[i].z, inv));
        int ijk[3];
        vx::unpack_cell(cells[i], ijk);
        for (int q = 0; q < 3; ++q) { imn[q] = std::min(imn[q], ijk[q]); imx[q] = std::max(imx[q], ijk[q]); }
      }
      vx::PackedBox pb;
      if (vx::make_packed_box(imn, imx, pb)) {
        ++n_decided;
        if (box.unfiltered) fail(c, "the integer guard decided a box PCL does not filter");
        const int bias[3] = {vx::kPackBiasXY, vx::kPackBiasXY, vx::kPackBiasZ};
        for (int q = 0; q < 3; ++q)
          if (pb.divc[q] != box.divb[q] || (float)(pb.minc[q] - bias[q]) != box.fminb[q]) fail(c, "packed box differs from the float box");
        if (vx::box_cells(pb.divc) != vx::box_cells(box.divb)) fail(c, "packed cell count differs");
        if (!box.unfiltered)
          for (int i = 0; i < n; ++i)
            if (vx::packed_cell_index(pb, cells[i]) != vx::cell_index(box, pts[i].x, pts[i].y, pts[i].z, inv)) { fail(c, "packed index differs from the float index"); break; }
      }
    }
    if (exact) {                                                              // run heads before the box is known: k_vox_lds
      ++n_exact;
      typedef unsigned __int128 wide;                                         // 3 x 23 bits of cell coordinates do not fit 64
      auto wide_index = [&](const P& p) {
        const wide i0 = (wide)(vx::cell_coord(p.x, inv) - box.fminb[0]), i1 = (wide)(vx::cell_coord(p.y, inv) - box.fminb[1]), i2 = (wide)(vx::cell_coord(p.z, inv) - box.fminb[2]);
        return i0 + i1 * (wide)box.divb[0] + i2 * (wide)box.divb[0] * (wide)box.divb[1];
      };
      for (int i = 0; i < n; ++i) {
        const wide wi = wide_index(pts[i]);
        if (!box.unfiltered && wi != (wide)vx::cell_index(box, pts[i].x, pts[i].y, pts[i].z, inv)) { fail(c, "wide index differs from cell_index in a filtered box"); break; }
        if (i == 0) continue;
        const P &p = pts[i], &q = pts[i - 1];
        const bool differs = vx::cell_differs(vx::cell_coord(p.x, inv), vx::cell_coord(p.y, inv), vx::cell_coord(p.z, inv),
                                              vx::cell_coord(q.x, inv), vx::cell_coord(q.y, inv), vx::cell_coord(q.z, inv));
        if (differs != (wi != wide_index(q))) { fail(c, "cell_differs disagrees with the index"); break; }
      }
    }
  }
  std::printf("%s: %d clouds, %lld points, %d unfiltered, %d decided by the integer path, %d with border points, %d with exact floors, %d failures\n",
              g_failures ? "voxel_device != pcl::VoxelGrid" : "voxel_device == pcl::VoxelGrid", kClouds, n_points, n_unfiltered, n_decided, n_border, n_exact, g_failures);
  if (n_unfiltered < 100 || n_decided < 500 || n_border < 100) { std::printf("a branch was taken too rarely\n"); return 2; }
  return g_failures ? 1 : 0;
}
