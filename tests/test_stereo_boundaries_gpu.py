"""stereo_rows / stereo_match / stereo_median on the constructed pairs of
stereo_boundary_scenario.py: on every case both sides' keypoints and
descriptors equal the oracle's, u_right and depth are byte-identical to the oracle's, and the
device error word carries no overflow. test_stereo_boundaries.py shows on the CPU that on these
cases every comparison of ComputeStereoMatches decides the designated keypoints' results, and
that the oracle equals an independent restatement; each case's precondition is asserted again
here, on the keypoints the device is compared with.

Every case runs through the single-frame call (the 1024-thread row-table and median kernels, the
packed record), through one batched launch per distinct camera with all that camera's cases as
frames, and through the same batches with a row pitch of cols + 1, where level-0 rows are not
4-byte aligned (the byte-wise window loads); the images, and with them the preconditions, are the
same at both pitches. The runtime takes the 256-thread row-table and median kernels only for more
than 8 frames (launch_stereo), so a camera's cases are repeated in turn until its batch has at
least BATCH_FRAMES frames, and every copy is compared."""
import numpy as np
import pytest

import stereo_boundary_scenario as B
from test_stereo_boundaries import evaluate

pytestmark = pytest.mark.gpu

CAMERAS = sorted({c.camera for c in B.CASES.values()})
BATCH_FRAMES = 9  # more than launch_stereo's threshold of 8 frames for the 1024-thread kernels


def camera(case):
    fx, bf = case.camera
    return (fx, fx, B.COLS / 2, B.ROWS / 2, bf)


def precondition(oracle, name):
    e = evaluate(oracle, name)
    B.check(B.CASES[name], e["kl"], e["dl"], e["kr"], e["dr"], e["ref_ur"], e["ref_depth"],
            e["trace"], e["scale"], e["inv_scale"])
    return e


def compare(ctx, e, frame, what):
    for side, (k, d) in enumerate(((e["kl"], e["dl"]), (e["kr"], e["dr"]))):
        kg, dg = ctx.keypoints(2 * frame + side)
        assert kg.tobytes() == k.tobytes(), f"{what}: keypoints of side {side}"
        assert np.array_equal(dg, d), f"{what}: descriptors of side {side}"
    gur, gdepth = ctx.stereo(frame)
    assert gur.tobytes() == e["ur"].tobytes(), f"{what}: u_right"
    assert gdepth.tobytes() == e["depth"].tobytes(), f"{what}: depth"


def no_device_error(G, ctx):
    ctx.sync()
    assert b"overflow" not in G.lib().slamgpu_last_error(ctx.h)


@pytest.mark.parametrize("name", list(B.CASES))
def test_single_frame(oracle, gpu_lib, name):
    e = precondition(oracle, name)
    ctx = gpu_lib.Context(B.COLS, B.ROWS, *B.ORB)
    ctx.frame_stereo(e["left"], e["right"], camera(B.CASES[name]))
    compare(ctx, e, 0, name)
    no_device_error(gpu_lib, ctx)


@pytest.mark.parametrize("pitch", [B.COLS, B.COLS + 1])
@pytest.mark.parametrize("cam", CAMERAS, ids=lambda c: f"fx{c[0]:g}")
def test_batch(oracle, gpu_lib, cam, pitch):
    """All cases of one camera as the frames of one launch of the 256-thread batch kernels."""
    import torch
    names = [n for n, c in B.CASES.items() if c.camera == cam]
    names = [names[f % len(names)] for f in range(max(len(names), BATCH_FRAMES))]
    evals = [precondition(oracle, n) for n in names]
    assert (pitch % 4 != 0) == (pitch != B.COLS)
    n, size = len(names), B.ROWS * pitch
    assert n > 8, "8 frames or fewer run on the single-frame call's 1024-thread kernels"
    host = np.zeros((2, n, B.ROWS, pitch), np.uint8)
    for f, e in enumerate(evals):
        host[0, f, :, :B.COLS] = e["left"]
        host[1, f, :, :B.COLS] = e["right"]
    d = torch.from_numpy(host.reshape(-1)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    ctx = gpu_lib.Context(B.COLS, B.ROWS, *B.ORB, max_frames=n)
    base = int(d.data_ptr())
    ctx.frontend_device(base, base + n * size, size, pitch, n, camera(B.CASES[names[0]]))
    no_device_error(gpu_lib, ctx)
    for f, (name, e) in enumerate(zip(names, evals)):
        compare(ctx, e, f, f"pitch {pitch}, frame {f} ({name})")
    no_device_error(gpu_lib, ctx)
