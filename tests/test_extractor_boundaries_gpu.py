"""The HIP extractor on the constructed images of extractor_boundary_scenario.py (DESIGN.md
section 4): every pyramid level, the FAST candidates and the octree output of every level,
keypoints and descriptors equal the oracle's bytes, and the device error word carries no overflow.
test_extractor_boundaries.py shows on the CPU that on these images every comparison of
ORBextractor decides the output and that the oracle equals an independent restatement; each case's
precondition is asserted again here.

Four paths, chosen by the thresholds the runtime documents (a test cannot see which kernel ran;
it asserts the condition the choice is made on):
  single   Context.extract: one image, octree_lvl_kernel (n_images <= OCT_LVL_MAX_IMAGES = 16),
           with debug_level_keys stages 0 and 1 and pyramid_level per level
  batch    frontend_device with 9 frames = 18 images (> 16: octree_img_kernel, the batched FAST
           and orient_desc kernels), the cases of one size and parameter set repeated in turn, at
           a 64-byte-multiple pitch (the LDS-staged pyramid)
  pitch    the same batches at pitch cols + 1 (cols + 2 where that is a multiple of 4): rows are
           not 4-byte aligned (the register-staged pyramid, byte-wise window loads)
  double   the cases of the common parameter set under twice the feature budget, 8 frames = 16
           images in one launch: octree_lvl_kernel with more than one image per launch. (At these
           image sizes a doubled budget does not overflow the per-image kernel's LDS, which is
           what sends KITTI-sized batches there; the batch size does.)"""
import numpy as np
import pytest

import extractor_boundary_scenario as B
from test_extractor_boundaries import evaluate

pytestmark = pytest.mark.gpu

OCT_LVL_MAX_IMAGES = 16  # orb_octree.hip
BATCH_FRAMES = 9
GROUPS = {}
for _c in B.CASES.values():
    GROUPS.setdefault((_c.size, _c.orb), []).append(_c.name)


def precondition(oracle, name):
    e = evaluate(oracle, name)
    for check in B.CASES[name].expect:
        check(B.CASES[name], e["rk"], e["rd"], e["trace"])
    return e


def no_device_error(G, ctx):
    ctx.sync()
    assert b"overflow" not in G.lib().slamgpu_last_error(ctx.h)


def compare_image(ctx, image, e, what, levels_from=1):
    for l in range(levels_from, len(e["levels"])):
        assert ctx.pyramid_level(image, l).tobytes() == e["levels"][l].tobytes(), \
            f"{what}: pyramid level {l}"
    kg, dg = ctx.keypoints(image)
    assert kg.tobytes() == e["k"].tobytes(), f"{what}: keypoints"
    assert dg.tobytes() == e["d"].tobytes(), f"{what}: descriptors"


@pytest.mark.parametrize("name", list(B.CASES))
def test_single_frame(oracle, gpu_lib, name):
    e = precondition(oracle, name)
    c = B.CASES[name]
    ctx = gpu_lib.Context(c.size[0], c.size[1], *c.orb)
    kg, dg = ctx.extract(e["img"])
    for l in range(len(e["levels"])):
        assert ctx.pyramid_level(0, l).tobytes() == e["levels"][l].tobytes(), f"level {l}"
        assert ctx.debug_level_keys(0, l, 0).tobytes() == \
            oracle.pack_keys(e["cand"][l]).tobytes(), f"FAST candidates of level {l}"
        assert ctx.debug_level_keys(0, l, 1).tobytes() == \
            oracle.pack_keys(e["octo"][l]).tobytes(), f"octree output of level {l}"
    assert kg.tobytes() == e["k"].tobytes(), "keypoints"
    assert dg.tobytes() == e["d"].tobytes(), "descriptors"
    no_device_error(gpu_lib, ctx)


def run_batch(oracle, gpu_lib, size, orb, names, pitch, evals):
    """Frame f holds case names[f] on the left and names[f + 1] on the right."""
    import torch
    cols, rows = size
    n = len(names)
    host = np.zeros((2, n, rows, pitch), np.uint8)
    for f in range(n):
        host[0, f, :, :cols] = evals[f]["img"]
        host[1, f, :, :cols] = evals[(f + 1) % n]["img"]
    d = torch.from_numpy(host.reshape(-1)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    ctx = gpu_lib.Context(cols, rows, *orb, max_frames=n)
    base, frame = int(d.data_ptr()), rows * pitch
    cam = (0.8 * cols, 0.8 * cols, cols / 2, rows / 2, 0.4 * cols)
    ctx.frontend_device(base, base + n * frame, frame, pitch, n, cam)
    no_device_error(gpu_lib, ctx)
    for f in range(n):
        compare_image(ctx, 2 * f, evals[f], f"pitch {pitch}, frame {f} left ({names[f]})")
        g = (f + 1) % n
        compare_image(ctx, 2 * f + 1, evals[g], f"pitch {pitch}, frame {f} right ({names[g]})")
    no_device_error(gpu_lib, ctx)


@pytest.mark.parametrize("aligned", [True, False], ids=["pitch64", "pitch_odd"])
@pytest.mark.parametrize("group", list(GROUPS), ids=lambda g: f"{g[0][0]}x{g[0][1]}-" + "-".join(
    f"{v:g}" for v in g[1][:3]))
def test_batch(oracle, gpu_lib, group, aligned):
    size, orb = group
    names = GROUPS[group]
    names = [names[f % len(names)] for f in range(max(len(names), BATCH_FRAMES))]
    assert 2 * len(names) > OCT_LVL_MAX_IMAGES, "the per-image octree kernel needs more images"
    pitch = (size[0] + 63) // 64 * 64 if aligned else size[0] + (1 if (size[0] + 1) % 4 else 2)
    assert (pitch % 64 == 0) == aligned and (aligned or pitch % 4 != 0)
    run_batch(oracle, gpu_lib, size, orb, names, pitch, [precondition(oracle, n) for n in names])


def test_batch_double_budget(oracle, gpu_lib):
    """Eight 282 x 132 cases under twice the budget of `levels` (the case whose budget binds on
    every level): the oracle runs them with the doubled budget too."""
    names = ["levels", "count_17", "count_stall", "fast", "angles", "descriptor", "blur_border",
             "saturated"]
    size, orb = B.CASES["levels"].size, B.CASES["levels"].orb
    assert all(B.CASES[n].size == size for n in names)
    assert 2 * len(names) <= OCT_LVL_MAX_IMAGES
    orb2 = (2 * orb[0],) + orb[1:]
    t = oracle.tables(*orb2)
    evals = []
    for n in names:
        img = B.CASES[n].image()
        k, d, pyr = oracle.extract(t, img, with_pyramid=True)
        evals.append(dict(img=img, k=k, d=d, levels=[pyr.level(l) for l in range(t.nlevels)]))
    assert any(len(e["k"]) != len(evaluate(oracle, n)["k"]) for n, e in zip(names, evals)), \
        "the doubled budget changes no case"
    run_batch(oracle, gpu_lib, size, orb2, names, (size[0] + 63) // 64 * 64, evals)
