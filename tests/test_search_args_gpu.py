"""The four batched searches (slamgpu_search_by_projection_{frame,mps,reloc}_device and
slamgpu_search_for_initialization_device) share one argument check: a null query range, record or
output pointer, a null query array when a frame can have a query, and a negative query count are
SLAMGPU_EINVAL before any launch, with the outputs untouched. A call without queries may still
pass a null query array, as it always could."""
import ctypes as C
import os

import numpy as np
import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EINVAL = -1
MP, BLK, NM, PREV, M12 = 41, 42, -77, 7.5, 43   # what the output buffers hold before a call


@pytest.mark.gpu
def test_device_searches_refuse_null_arguments(gpu_lib):
    import torch
    G = gpu_lib
    L = G.lib()
    img = np.load(os.path.join(HERE, "orb_small_320x240.npz"))["image"]
    ctx = G.Context(320, 240, nfeatures=500)
    ctx.frame_stereo(img, img, (300.0, 300.0, 160.0, 120.0, 30.0))
    kc = ctx.kp_cap
    dev = torch.device("cuda", 0)
    zeros = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=dev)  # noqa: E731
    # one frame with an empty query list: a call that passes the check launches next to nothing
    d_q, d_pose = zeros(80), zeros(72)
    d_qs = torch.zeros(1, dtype=torch.int32, device=dev)
    d_qc = torch.zeros(1, dtype=torch.int32, device=dev)
    out = dict(mp=torch.full((kc,), MP, dtype=torch.int32, device=dev),
               blk=torch.full((kc,), BLK, dtype=torch.uint8, device=dev),
               nm=torch.full((1,), NM, dtype=torch.int32, device=dev),
               prev=torch.full((2,), PREV, dtype=torch.float32, device=dev),
               m12=torch.full((1,), M12, dtype=torch.int32, device=dev))

    def untouched():
        torch.cuda.synchronize()
        return bool((out["mp"] == MP).all() and (out["blk"] == BLK).all() and
                    (out["prev"] == PREV).all() and (out["m12"] == M12).all())

    P = lambda t: C.c_void_p(int(t.data_ptr()))  # noqa: E731
    st = C.c_void_p(0)
    # (entry, its arguments after the context by name, the pointers that may never be null, the
    # pointers needed only when max_queries > 0)
    proj = dict(q=P(d_q), total=0, qs=P(d_qs), qc=P(d_qc), maxq=1, pose=P(d_pose),
                mp=P(out["mp"]), blk=P(out["blk"]), stride=kc, nm=P(out["nm"]), nf=1, st=st)
    order = ("q", "total", "qs", "qc", "maxq", "pose", "mp", "blk", "stride", "nm", "nf", "st")
    entries = [
        (L.slamgpu_search_by_projection_frame_device, proj, order,
         ("qs", "qc", "pose", "mp", "blk", "nm"), ("q",)),
        (L.slamgpu_search_by_projection_reloc_device, proj, order,
         ("qs", "qc", "pose", "mp", "blk", "nm"), ("q",)),
        (L.slamgpu_search_by_projection_mps_device, dict(proj, nnratio=0.8, th=1),
         ("q", "total", "qs", "qc", "maxq", "nnratio", "th", "mp", "blk", "stride", "nm", "nf", "st"),
         ("qs", "qc", "mp", "blk", "nm"), ("q",)),
        (L.slamgpu_search_for_initialization_device,
         dict(q=P(d_q), total=0, qs=P(d_qs), qc=P(d_qc), maxq=1, pose=P(d_pose),
              prev=P(out["prev"]), m12=P(out["m12"]), nm=P(out["nm"]), nf=1, st=st),
         ("q", "total", "qs", "qc", "maxq", "pose", "prev", "m12", "nm", "nf", "st"),
         ("qs", "qc", "pose", "nm"), ("q", "prev", "m12")),
    ]
    for fn, args, names, always, with_queries in entries:
        call = lambda **kw: fn(ctx.h, *[dict(args, **kw)[k] for k in names])  # noqa: E731
        for name in always + with_queries:
            assert call(**{name: None}) == EINVAL, (fn.__name__, name)
            assert b"bad arguments" in L.slamgpu_last_error(ctx.h)
            assert untouched() and int(out["nm"][0]) == NM, (fn.__name__, name)
        for name in always:   # ... whether or not a frame can have a query
            assert call(maxq=0, **{name: None}) == EINVAL, (fn.__name__, name)
        assert call(total=-1) == EINVAL and call(maxq=-1) == EINVAL, fn.__name__
        assert untouched() and int(out["nm"][0]) == NM, fn.__name__
        assert fn(None, *[args[k] for k in names]) == EINVAL
        # no query anywhere: the query-side arrays may be null, and the call runs
        assert call(maxq=0, **{name: None for name in with_queries}) == 0, fn.__name__
        assert untouched() and int(out["nm"][0]) == 0, fn.__name__
        out["nm"].fill_(NM)
