// orb_extract.hip -- the ORBextractor::Compute hot path as gfx950 kernels, batched over images.
//
// Pipeline for a batch of n images (all levels of all images in flight together), one stage per
// file, each opening with its own paragraph:
//   pyr_down      orb_pyramid.hip      level l from level l-1 (resize INTER_LINEAR 8U)
//   fast_cells    orb_fast.hip         per-cell FAST-9 score, threshold fallback, cell NMS
//                                      (batches: level 0 on a side stream beside the pyramid)
//   octree        orb_octree.hip       DistributeOctTree, exact list / pointer-order semantics
//   orient_desc   orb_orient_desc.hip  IC_Angle + 7x7-blurred rBRIEF, ORBextractor::Compute order
// Reference: src/orb_features/orb_extractor.cpp (citations per kernel). Built with
// -ffp-contract=off; fused multiply-adds are explicit where the reference's Release build fuses.
#include "orb_stages.h"

namespace slamgpu {

void launch_extract(const ImageBatch& b, const OrbGeomDev& gd, int n_images, hipStream_t st,
                    const ExtractStreams& fx) {
  const OrbGeom& g = *gd.host;
  // glds tiles need every cell view 16-byte aligned: the caller's level-0 images included
  const bool glds = ((reinterpret_cast<uintptr_t>(b.in_l) | reinterpret_cast<uintptr_t>(b.in_r) |
                      (uintptr_t)b.in_stride | (uintptr_t)b.in_pitch |
                      reinterpret_cast<uintptr_t>(b.pyr) | (uintptr_t)g.pyr_bytes) & 15) == 0;
  // FAST of level 0 reads only the caller's images: with a second side stream it runs beside
  // the pyramid (whose small levels leave the chip mostly idle)
  // (batches only: in the single-frame call the join's cross-queue dependency costs more than
  // the overlap saves -- 0.296 -> 0.276 ms per call without it, profiles/r4w_lat_ab.log)
  const bool split0 = fx.side0 && fx.fork0 && fx.join0 && g.nlevels > 1 &&
                      n_images > kPyrShortMaxImages;
  const int level1 = split0 ? g.lv[1].cell_base : 0;  // the first cell not run on the side stream
  if (split0) {
    (void)hipEventRecord(fx.fork0, st);
    (void)hipStreamWaitEvent(fx.side0, fx.fork0, 0);
    launch_fast_cells(b, gd, n_images, 0, level1, fx.side0, glds);
    (void)hipEventRecord(fx.join0, fx.side0);
  }
  launch_pyramid(b, gd, n_images, st, glds);
  launch_fast_cells(b, gd, n_images, level1, g.cells_per_image, st, glds);
  if (split0) (void)hipStreamWaitEvent(st, fx.join0, 0);
  launch_octree(gd, n_images, st);
  launch_orient_desc(b, gd, n_images, st);
}

bool extract_build_matches(const OrbGeom& g) {
  return pyramid_build_matches(g) && fast_build_matches(g);
}

}  // namespace slamgpu
