"""The rule of query._OnStream for memory, on a side stream given as a torch.cuda.Stream and as its raw handle: a tensor a call
allocates and does not return belongs to the call's stream, so torch's allocator cannot hand its block to the current stream while the
call is still queued.  Three calls have such a temporary -- winding_number's accumulator where fixed=False (chunks=2: memset, atomic
adds and a finishing kernel, all on the stream), plane_count's per-slice counts, and the overlap lists' n_overlap where a capacity is
given (nothing synchronises) -- and each is run on the voxel solid of tests/inside_scenes.py with 65 queries:

* the side stream first sleeps (about 20 ms), and the call is enqueued behind the sleep;
* as soon as the call has returned, and before anything synchronises, tensors of the temporaries' sizes are allocated on the
  current stream and filled with a pattern: the blocks a freed temporary would have gone to;
* after torch.cuda.synchronize() the answer is the default stream's on the bits and every filler still holds its pattern.

Nothing here can fault: the worst outcome is wrong numbers in these tensors.  What the wrappers did before _OnStream: profiles/r40/."""
import os
import sys

import numpy as np
import pytest

from ezrt_amd import query

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inside_scenes as IS  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N = 65
SLEEP = 40_000_000                                                     # cycles: about 20 ms
FILLERS = 16
PATTERN = 0x5A


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def solid(hip, dev):
    """(the device scene, points [65, 3], planes [65, 4], lo and hi [65, 3]) on the device, and the default stream's answers"""
    v = IS.voxel_solid()
    sg = hip.scene_create(v["tri"], v["nodes"])
    p = v["points"][np.linspace(0, v["points"].shape[0] - 1, N).astype(np.int64)].astype(np.float32)
    nrm = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 2, 3]], np.float32)[np.arange(N) % 5]
    planes = np.concatenate([nrm, (nrm * p).sum(1, keepdims=True)], 1).astype(np.float32)
    gpu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    inputs = dict(points=gpu(p), planes=gpu(planes), lo=gpu(p - 0.75), hi=gpu(p + 0.75))
    first = query.box_overlap_list(sg, inputs["lo"], inputs["hi"])     # the first, synchronising call: the capacity of the second
    capacity = int(first.offsets[N].item())
    assert capacity > 0
    calls = {
        "winding": (lambda s: (query.winding_number(sg, inputs["points"], fixed=False, chunks=2, stream=s),), [(N,)], torch.int64),
        "plane_count": (lambda s: (query.plane_count(sg, inputs["planes"], slices=2, stream=s),), [(N, 2)], torch.int32),
        "box_list": (lambda s: query.box_overlap_list(sg, inputs["lo"], inputs["hi"], capacity=capacity, stream=s)[:2], [(N,)], torch.int32),
    }
    want = {name: [x.clone() for x in run(None)] for name, (run, _, _) in calls.items()}
    torch.cuda.synchronize()
    assert want["winding"][0].abs().max() > 0.9 and want["plane_count"][0].max() > 0 and torch.equal(want["box_list"][1], first.tri)
    return calls, want


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


@pytest.mark.parametrize("raw", (False, True), ids=("torch_stream", "raw_handle"))
@pytest.mark.parametrize("name", ("winding", "plane_count", "box_list"))
def test_temporaries_belong_to_the_calls_stream(solid, dev, name, raw):
    calls, want = solid
    run, shapes, dtype = calls[name]
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()                                           # a freed temporary is then the next block of its size
    with torch.cuda.stream(side):
        torch.cuda._sleep(SLEEP)
    got = run(side.cuda_stream if raw else side)
    fillers = [torch.full(shape, PATTERN, dtype=dtype, device=dev) for shape in shapes for _ in range(FILLERS)]
    torch.cuda.synchronize()
    assert len(got) == len(want[name])
    for g, w in zip(got, want[name]):
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(_bits(g), _bits(w)), name
    for f in fillers:
        assert bool((f == PATTERN).all()), "%s: a block of the call's temporary was handed to the current stream" % name
