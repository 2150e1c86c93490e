"""GPU: the training march's count pass follows the jumps of a ray by pointer doubling (csrc/raymarching.hip, march_count_parallel_kernel).

Every case is compared for EXACT equality -- counter, ray records, sample rows up to the total, zeros behind it -- with the oracle's serial loop
and with the library's own one-ray-per-lane kernel (`march_serial` knob).  The grids are chosen for what the walk has to do on them: paths of 128
hops (every doubling round), jumps of 1-3, nothing but skips carried across segment boundaries, the max_steps cap inside a later segment; the batch
sizes for ragged workgroups of the 32-rays-per-workgroup kernel.  What each grid gives was confirmed with the oracle on the CPU (N = 97, perturb
off): see CASES and EXPECT_97.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND, H, DT_GAMMA = 2.0, 128, 1 / 128


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_scene = {}


def _grid(name):
    """Occupancy bitfields of C * H^3 bits."""
    from ngp_harness import scene

    if "sc" not in _scene:
        sc = scene.Scene(bound=BOUND, seed=1)
        _scene["sc"] = sc
        _scene["scene"] = np.ascontiguousarray(sc.bitfield()[2], dtype=np.uint8)
    nbytes = _scene["sc"].cascade * H ** 3 // 8
    if name not in _scene:
        if name == "ones":
            g = np.full(nbytes, 0xFF, np.uint8)
        elif name == "zeros":
            g = np.zeros(nbytes, np.uint8)
        elif name == "alternate":
            g = np.full(nbytes, 0x55, np.uint8)
        else:
            assert name == "sparse"
            g = np.packbits(np.random.default_rng(3).random(nbytes * 8) < 1 / 64, bitorder="little")
        _scene[name] = g
    assert _scene[name].shape == (nbytes,)
    return _scene[name], _scene["sc"].cascade


# grid, max_steps, what it exercises
CASES = [
    ("scene", 1024),      # 348-383 members per ray: three segments, skips across both boundaries
    ("ones", 1024),       # 128-hop paths, every doubling round needed
    ("ones", 160),        # the cap falls inside the second segment
    ("ones", 32),         # dt_min > dt_max, one segment, every ray at the cap
    ("zeros", 1024),      # nothing but skips and pending carries
    ("alternate", 1024),  # jumps of 1-3
    ("sparse", 1024),     # long skips
]

# oracle, N = 97, perturb off: (samples, rays without a sample, most samples on a ray, rays that stop at max_steps)
EXPECT_97 = {("scene", 1024): (6678, 14, 150, 0), ("ones", 1024): (35170, 0, 383, 0), ("ones", 160): (15512, 0, 160, 89), ("ones", 32): (3104, 0, 32, 97),
             ("zeros", 1024): (0, 97, 0, 0), ("alternate", 1024): (17502, 0, 203, 0), ("sparse", 1024): (606, 7, 24, 0)}

_ref = {}


def _reference(oracle, grid_name, max_steps, N, perturb, seed=5):
    """rays, near / far and the oracle's march: computed once per case, shared, never modified."""
    key = (grid_name, max_steps, N, perturb, seed)
    if key not in _ref:
        from ngp_harness import scene

        bits, C = _grid(grid_name)
        o, d = scene.train_batch(N, seed=seed)
        aabb = np.array([-BOUND] * 3 + [BOUND] * 3, np.float32)
        nears, fars = oracle.near_far_from_aabb(o, d, aabb, 0.2)
        M = (N * min(max_steps, 384) + 4) // 4 * 4  # no ray has more than 384 sequence members inside the box: nothing is dropped
        want = oracle.march_rays_train(o, d, BOUND, bits, C, H, nears, fars, M, perturb, DT_GAMMA, max_steps)
        for a in (o, d, nears, fars, *want[:5]):
            a.setflags(write=False)
        _ref[key] = (o, d, nears, fars, M, want)
    return _ref[key]


def _march(dev, grid_name, max_steps, perturb, o, d, nears, fars, M):
    import raymarching

    bits, C = _grid(grid_name)
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)  # noqa: E731
    counter = torch.zeros(2, dtype=torch.int32, device=dev)
    out = raymarching.march_rays_train(t(o), t(d), BOUND, t(bits), C, H, t(nears), t(fars), counter, M, perturb, -1, False, DT_GAMMA, max_steps)
    return out, counter


def _assert_same(got, counter, want, M):
    xyzs, dirs, deltas, rays = (a.cpu().numpy() for a in got)
    wx, wd, wl, wr, wc = want[:5]
    assert xyzs.shape[0] == M
    assert counter.cpu().tolist() == wc.tolist()
    assert np.array_equal(rays, wr)
    m = int(wc[0])
    for a, w in ((xyzs, wx), (dirs, wd), (deltas, wl)):
        assert np.array_equal(a[:m].view(np.uint32), w[:m].view(np.uint32))
        assert not a[m:].any()


@pytest.mark.parametrize("perturb", [False, True])
@pytest.mark.parametrize("N", [97, 31, 33])
@pytest.mark.parametrize("grid_name,max_steps", CASES)
def test_count_pass_walk_matches_the_serial_loop(oracle, dev, knobs, grid_name, max_steps, N, perturb):
    o, d, nears, fars, M, want = _reference(oracle, grid_name, max_steps, N, perturb)
    total, per_ray = int(want[4][0]), want[3][:, 2]
    print(f"{grid_name} max_steps={max_steps} N={N} perturb={perturb}: {total} samples, {int((per_ray == 0).sum())} empty rays, "
          f"most {int(per_ray.max())}, at the cap {int((per_ray == max_steps).sum())}")
    if N == 97 and not perturb:  # the case exercises what it names
        assert (total, int((per_ray == 0).sum()), int(per_ray.max()), int((per_ray == max_steps).sum())) == EXPECT_97[(grid_name, max_steps)]
    got, counter = _march(dev, grid_name, max_steps, perturb, o, d, nears, fars, M)
    _assert_same(got, counter, want, M)
    knobs(march_serial=1)
    got, counter = _march(dev, grid_name, max_steps, perturb, o, d, nears, fars, M)
    _assert_same(got, counter, want, M)


def test_two_marches_back_to_back_share_nothing(oracle, dev):
    """Two launches on one stream into the same scratch, different rays, grids and sizes, nothing waited for in between: what a captured step and the
    march that runs ahead of it do.  No LDS or workspace state of the first may show in the second."""
    a = _reference(oracle, "ones", 1024, 97, True)
    b = _reference(oracle, "scene", 1024, 33, True, seed=6)
    c = _reference(oracle, "zeros", 1024, 97, False)
    got = [_march(dev, g, 1024, p, r[0], r[1], r[2], r[3], r[4]) for g, p, r in (("ones", True, a), ("scene", True, b), ("zeros", False, c), ("scene", True, b))]
    for (out, counter), r in zip(got, (a, b, c, b)):
        _assert_same(out, counter, r[5], r[4])
