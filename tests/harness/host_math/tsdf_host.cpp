// TEST INFRASTRUCTURE (tests/test_tsdf_rule_on_host.py): the PRODUCT's csrc/tsdf_rule.h -- copied next to this file at
// test time, never edited -- compiled for the host; its "common.h" is the stand-in beside this file.
#include "tsdf_rule.h"

// n samples at lattice indices ijk [n,3] of a volume (lo, voxel), each under its own view: the 17 words of row r of
// `views` are view[12], tanfovx, tanfovy, z_min, W, H (the last two as floats holding integers).  Outputs: seen [n]
// (steps 1 and 2 passed), z [n], pix [n,2]; then, with d / w / rgb [n,3] as read at the pixel, the update in place on
// tsdf, weight, colour [n,3] (use_colour, use_rgb: whether the pointers are handed on) and applied [n].
extern "C" void host_tsdf_samples(const int32_t* ijk, int64_t n, const float* lo, float voxel, const float* views,
                                  const float* d, const float* w, const float* rgb, int32_t use_colour, int32_t use_rgb,
                                  float trunc, float max_weight, int32_t* seen, float* z, int32_t* pix, float* tsdf,
                                  float* weight, float* colour, int32_t* applied) {
  for (int64_t r = 0; r < n; ++r) {
    const float* v = views + r * 17;
    const float x0 = hgs::tsdf_lattice(lo[0], voxel, ijk[r * 3]), x1 = hgs::tsdf_lattice(lo[1], voxel, ijk[r * 3 + 1]),
                x2 = hgs::tsdf_lattice(lo[2], voxel, ijk[r * 3 + 2]);
    float zz = 0.0f;
    int32_t px = 0, py = 0;
    seen[r] = hgs::tsdf_project(x0, x1, x2, v, v[12], v[13], (int32_t)v[15], (int32_t)v[16], v[14], &zz, &px, &py) ? 1 : 0;
    z[r] = zz;
    pix[r * 2] = px;
    pix[r * 2 + 1] = py;
    applied[r] = 0;
    if (seen[r])
      applied[r] = hgs::tsdf_update(d[r], w[r], rgb + r * 3, use_colour && use_rgb, zz, trunc, max_weight, tsdf + r,
                                    weight + r, colour + r * 3) ? 1 : 0;
  }
}

// n cells: t, w [n,8], c [n,3,8] -> active [n], local, normal, colour [n,3], world [n,3] at cell ijk [n,3]
extern "C" void host_tsdf_cells(const float* t, const float* w, const float* c, const int32_t* ijk, int64_t n,
                                const float* lo, float voxel, float min_weight, int32_t* active, float* local,
                                float* normal, float* colour, float* world) {
  for (int64_t r = 0; r < n; ++r) {
    active[r] = hgs::tsdf_cell_active(t + r * 8, w + r * 8, min_weight) ? 1 : 0;
    if (!active[r]) continue;
    hgs::tsdf_cell_vertex(t + r * 8, local + r * 3, normal + r * 3);
    for (int a = 0; a < 3; ++a) {
      world[r * 3 + a] = hgs::tsdf_vertex_world(lo[a], voxel, ijk[r * 3 + a], local[r * 3 + a]);
      colour[r * 3 + a] = hgs::tsdf_cell_colour(c + (r * 3 + a) * 8);
    }
  }
}

// the four cell offsets around an edge along `axis` [4,3] and the two triangles of vertex indices v[4]
extern "C" void host_tsdf_quad(int32_t axis, const int32_t* v, int32_t lower_inside, int32_t* cells, int32_t* faces) {
  int32_t o[4][3];
  hgs::tsdf_quad_cells(axis, o);
  for (int q = 0; q < 4; ++q)
    for (int a = 0; a < 3; ++a) cells[q * 3 + a] = o[q][a];
  hgs::tsdf_quad_faces(v, lower_inside != 0, faces);
}
