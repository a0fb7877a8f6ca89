// orb_stages.h -- the extractor's stage launchers, one per orb_*.hip, as launch_extract
// (orb_extract.hip) chains them. Internal: only csrc/orb_*.hip include it.
#pragma once
#include "orb_kernels.h"

namespace slamgpu {

// Launches of up to this many images are "small" (the single-frame call): the pyramid takes
// short strips and row bands, and level 0's FAST does not fork to the side stream.
constexpr int kPyrShortMaxImages = 16;

// Each launcher issues its stage's kernels on `st`. glds: every cell view of the launch is
// 16-byte aligned (launch_extract). FAST runs the cells [lo, hi) of every image.
void launch_pyramid(const ImageBatch& b, const OrbGeomDev& gd, int n_images, hipStream_t st,
                    bool glds);
void launch_fast_cells(const ImageBatch& b, const OrbGeomDev& gd, int n_images, int lo, int hi,
                       hipStream_t st, bool glds);
void launch_octree(const OrbGeomDev& gd, int n_images, hipStream_t st);
void launch_orient_desc(const ImageBatch& b, const OrbGeomDev& gd, int n_images, hipStream_t st);

// Each stage's own build constants against the geometry's (extract_build_matches)
bool pyramid_build_matches(const OrbGeom& g);
bool fast_build_matches(const OrbGeom& g);

}  // namespace slamgpu
