// geometry_check.cpp -- compute_geometry / build_cells on the host, printed as JSON.
//
// Links slam_framework_amd/csrc/orb_geometry.cpp only: no device code, no GPU. One JSON line per
// configuration:
//   geometry_check [--lds IMG_BYTES LVL_BYTES] cols rows nfeatures scale nlevels [cols rows ...]
// --lds passes the octree kernels' dynamic LDS limits (default: none, as slamgpu_create without a
// usable device). tests/test_geometry.py checks the output against a restatement of the
// reference's formulas and the kernels' layout invariants.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orb_tables.h"

using namespace slamgpu;

static void one(int cols, int rows, int nf, float scale, int nlevels, int img_lds, int lvl_lds) {
  OrbParams p{nf, scale, nlevels, 20, 7};
  static OrbGeom g;
  std::vector<ResizeX> rx;
  std::vector<ResizeY> ry;
  const int rc = compute_geometry(p, cols, rows, &g, &rx, &ry, img_lds, lvl_lds);
  std::printf("{\"cols\":%d,\"rows\":%d,\"nfeatures\":%d,\"scale\":%.9g,\"nlevels\":%d,\"rc\":%d",
              cols, rows, nf, (double)scale, nlevels, rc);
  if (rc != 0) {
    std::printf("}\n");
    return;
  }
#define TOP(f) std::printf(",\"" #f "\":%lld", (long long)g.f)
  TOP(pyr_ring_strip); TOP(cell_group); TOP(cells_per_image); TOP(cell_cap);
  TOP(fast_tile_stride); TOP(fast_tile_rows); TOP(fast_score_stride); TOP(fast_score_rows);
  TOP(fast_lds_per_wave); TOP(pyr_bytes); TOP(keys_per_image); TOP(oct_lds_bytes); TOP(oct_kcap);
  TOP(oct2_lds_bytes); TOP(oct2_kcap); TOP(oct2_ccap); TOP(oct2_nc); TOP(oct2_tmp_off);
  TOP(oct2_cpre_off); TOP(oct2_list_off); TOP(oct2_work_off); TOP(out_per_image); TOP(kp_cap);
  TOP(pyr_bands); TOP(pyr_ring_slots); TOP(pyr_band_lds); TOP(casc_waves); TOP(casc_steps);
  TOP(casc_lds);
#undef TOP
  std::printf(",\"max_bands\":%d,\"lv\":[", kPyrMaxBands);
  for (int l = 0; l < g.nlevels; l++) {
    const LevelGeom& L = g.lv[l];
    std::printf("%s{\"hx\":%.9g", l ? "," : "", (double)L.hx);
#define LV(f) std::printf(",\"" #f "\":%lld", (long long)L.f)
    LV(w); LV(h); LV(pitch); LV(offset); LV(max_bx); LV(max_by); LV(ncols); LV(nrows); LV(wcell);
    LV(hcell); LV(cell_base); LV(budget); LV(n_ini); LV(node_cap); LV(key_cap); LV(key_base);
    LV(out_base); LV(out_cap); LV(oct_nc); LV(oct_list_off); LV(oct_work_off); LV(pyr_lpr);
    LV(pyr_rpi); LV(pyr_slots);
#undef LV
    std::printf(",\"ry\":[");  // source rows y0, y1 of every row of this level (level >= 1)
    for (int y = 0; l > 0 && y < L.h; y++)
      std::printf("%s%d,%d", y ? "," : "", ry[L.ry_base + y].y0, ry[L.ry_base + y].y1);
    std::printf("],\"band\":[");  // pyr_band_kernel's row range of every band
    for (int s = 0; s < g.pyr_bands; s++)
      std::printf("%s%d,%d", s ? "," : "", g.pyr_band[s][l][0], g.pyr_band[s][l][1]);
    std::printf("]}");
  }
  std::vector<CellDesc> cells;
  build_cells(g, &cells);
  std::printf("],\"cells\":[");  // level, ini_x, ini_y, vw, vh per cell, padding cells included
  for (size_t i = 0; i < cells.size(); i++)
    std::printf("%s%d,%d,%d,%d,%d", i ? "," : "", cells[i].level, cells[i].ini_x, cells[i].ini_y,
                cells[i].vw, cells[i].vh);
  std::printf("]}\n");
}

int main(int argc, char** argv) {
  int a = 1, img_lds = 1 << 30, lvl_lds = 1 << 30;
  if (argc >= 4 && !std::strcmp(argv[1], "--lds")) {
    img_lds = std::atoi(argv[2]);
    lvl_lds = std::atoi(argv[3]);
    a = 4;
  }
  if (argc - a < 5 || (argc - a) % 5) {
    std::fprintf(stderr, "usage: %s [--lds IMG LVL] cols rows nfeatures scale nlevels ...\n",
                 argv[0]);
    return 2;
  }
  for (; a + 5 <= argc; a += 5)
    one(std::atoi(argv[a]), std::atoi(argv[a + 1]), std::atoi(argv[a + 2]),
        std::strtof(argv[a + 3], nullptr), std::atoi(argv[a + 4]), img_lds, lvl_lds);
  return 0;
}
