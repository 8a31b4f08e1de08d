"""CPU side of the synthetic corridor cases (tests/synth_corridor.py).

1. The oracle's box test (oracle/corridor.c is_obstacle_in_box) is pinned against a plain numpy restatement of isObstacleInBox
   (rbp_corridor.hpp:44-78), written from the reference text, on every grid shape / resolution / origin of the case table -- boxes
   partly outside the grid included -- in the boolean AND in the number of getDistance calls.  Everywhere else it is only ever run at
   0.1 m on the 101 x 101 x 23 grid.
2. The generator keeps its promises, so that no GPU test of test_gpu_corridor_synthetic.py passes on a case that does not reach the
   branch it is named after: the oracle accepts every mission, the corridors have several boxes, paths hover and step back, every grid
   is on the intended side of the thresholds of kernels/corridor.hip and abi/session.hip.
"""
import numpy as np
import pytest

from tests import oracle_lib as O
from tests import synth_corridor as S

SFC_MASK_WORDS = 8192   # kernels/rbp_dev.h


def numpy_is_obstacle_in_box(world, param, box, margin):
    """rbp_corridor.hpp:44-78 restated: returns (hit, number of getDistance calls).  The loop variables accumulate (`v += res`), the first
    sample of an axis sits 1e-6 below the box unless the box starts at the world's edge, every other one 1e-6 above the loop variable;
    octomap::point3d is float32; DynamicEDTOctomap::getDistance looks up floor(coord / res_map) - key_min and answers -1 outside."""
    eps = 1e-6
    wmin = (param.world_x_min, param.world_y_min, param.world_z_min)
    step = (param.box_xy_res, param.box_xy_res, param.box_z_res)
    keys = []
    for a in range(3):
        coords, v, count = [], box[a], 0
        while v < box[a + 3] + eps:
            c = v + eps
            if count == 0 and box[a] > wmin[a] + eps:
                c = box[a] - eps
            coords.append(c)
            v += step[a]
            count += 1
        cf = np.array(coords, np.float64).astype(np.float32)
        keys.append(np.floor((1.0 / world.res) * cf.astype(np.float64)).astype(np.int64) - world.key_min[a])
    if any(len(k) == 0 for k in keys):
        return False, 0
    dim = world.dist.shape
    inside = [(k >= 0) & (k < dim[a]) for a, k in enumerate(keys)]
    d = np.full([len(k) for k in keys], -1.0, np.float32)
    sub = world.dist[np.ix_(*[k[i] for k, i in zip(keys, inside)])]
    d[np.ix_(*[np.flatnonzero(i) for i in inside])] = sub
    hit = (d.astype(np.float64) < margin - eps).reshape(-1)   # x outer, z inner: the reference's order
    if hit.any():
        return True, int(np.argmax(hit)) + 1   # early exit at the first hit
    return False, hit.size


def random_boxes(rng, world, param, n):
    """boxes on the box_res lattice (as updateObsBox / expand_box produce them), some far from it; inside, across and outside the grid"""
    glo, ghi = S.grid_extent(world)
    res = np.array([param.box_xy_res, param.box_xy_res, param.box_z_res])
    for i in range(n):
        lo = rng.uniform(glo - 0.4, ghi + 0.2)
        ext = rng.uniform(0.0, [1.2, 1.2, 0.8]) * (rng.random(3) < 0.8)   # zero extents: slabs and degenerate seed boxes
        if i % 4:
            lo, ext = np.round(lo / res) * res, np.round(ext / res) * res
        yield np.concatenate([lo, lo + ext])


@pytest.mark.parametrize("name", list(S.CASES))
def test_oracle_box_test_follows_the_reference_text(name):
    c = S.CASES[name]
    s = S.missions(name)[0]
    rng = np.random.default_rng([77, list(S.CASES).index(name)])
    n_hit = n_free = n_out = 0
    for box in random_boxes(rng, s.world, s.param, 300):
        margin = float(rng.choice(c.radius))
        want = numpy_is_obstacle_in_box(s.world, s.param, box, margin)
        got = O.is_obstacle_in_box(s.world, s.param, box, margin)
        assert got == want, (name, box.tolist(), margin, got, want)
        n_hit += want[0]
        n_free += not want[0]
        glo, ghi = S.grid_extent(s.world)
        n_out += bool(np.any(box[:3] < glo) or np.any(box[3:] > ghi))
    assert n_hit >= 30 and n_free >= 30 and n_out >= 30, (n_hit, n_free, n_out)   # both answers and the grid's edge are exercised


def test_expand_box_wrapper_grows_a_free_seed_to_a_free_box():
    s = S.missions("coarse_box")[0]
    seed = S.seed_box(s.plan.init_traj[0, 0], s.plan.init_traj[0, 1], s.param)
    assert not O.is_obstacle_in_box(s.world, s.param, seed, 0.15)[0]
    box = O.expand_box(s.world, s.param, seed, 0.15)
    assert np.all(box[:3] <= seed[:3]) and np.all(box[3:] >= seed[3:]) and np.any(box != seed)
    assert not O.is_obstacle_in_box(s.world, s.param, box, 0.15)[0]


def test_c_round_goes_away_from_zero_on_ties():
    assert [S.c_round(v) for v in (2.5, -2.5, 0.5, -0.5, 3.5, 0.49999999999999994, 2.4999999999999996)] == [3, -3, 1, -1, 4, 0, 2]
    assert np.round(2.5) == 2   # what the generator must not use


@pytest.mark.parametrize("name", list(S.CASES))
def test_generator_keeps_its_promises(name):
    c = S.CASES[name]
    ms, refs = S.missions(name), S.reference(name)
    assert len(ms) == len(S.SEEDS) == 3
    assert [r[0] for r in refs] == [0, 0, 0]
    counts = np.concatenate([r[2].sfc_count for r in refs])
    assert counts.mean() >= 3 and counts.max() >= 6 and counts.min() >= 1, counts
    hover = back = 0
    for s in ms:
        t = s.plan.init_traj
        assert t.dtype == np.float32 and t.shape == (c.N, c.M + 1, 3) and np.array_equal(s.plan.T, np.arange(c.M + 1))
        assert np.abs(np.diff(t.astype(np.float64), axis=1)).max() <= S.MAX_STEP
        same = np.all(t[:, 1:] == t[:, :-1], axis=2)
        hover += int(same.sum())
        back += int((np.all(t[:, 2:] == t[:, :-2], axis=2) & ~same[:, 1:]).sum())
        for i in range(c.M):   # no pair's relative segment comes near the origin (RBP_ERR_INIT_TRAJ_COLLIDE is a case of its own)
            for a in range(c.N):
                for b in range(a + 1, c.N):
                    d0, d1 = (t[b, i].astype(np.float64) - t[a, i]), (t[b, i + 1].astype(np.float64) - t[a, i + 1])
                    assert S.closest_approach(d0, d1) >= S.MIN_APPROACH
        if c.snap:
            assert np.array_equal(np.round(t.astype(np.float64) / c.snap) * c.snap, t.astype(np.float64))
        else:
            assert np.abs(t / 0.05 - np.round(t / 0.05)).max() > 0.1   # off the lattice
    assert hover >= 1 and back >= 1, (hover, back)


def mask_words(dim):
    nc = dim[0] * dim[1] * dim[2]
    return ((((nc + 63) >> 6) * 2 + 2) + 3) & ~3   # abi/session.hip: words of the bitmask, one word past the last cell, 16-byte quads


@pytest.mark.parametrize("name", list(S.CASES))
def test_grids_are_on_the_intended_side_of_each_threshold(name):
    c = S.CASES[name]
    for s in S.missions(name):
        assert s.world.dist.shape == c.dim and s.world.dist.dtype == np.float32 and s.world.res == c.res
        assert float(s.world.dist.max()) <= 1.0 and float(s.world.dist.min()) == 0.0
    words, ncell = mask_words(c.dim), c.dim[0] * c.dim[1] * c.dim[2]
    fits = words <= SFC_MASK_WORDS
    assert fits == (ncell + 64 <= 32 * SFC_MASK_WORDS)   # mask_kernel's test and the session's agree
    if name == "mask_first_off":
        assert not fits and mask_words((64, 65, 63)) == SFC_MASK_WORDS and ncell == 262144
    else:
        assert fits
    if name == "mask_last":
        assert ncell == 262080 and words == SFC_MASK_WORDS and c.dim[2] > 32
    want_z = {"column_23": 23, "column_32": 32, "generic_33": 33, "generic_41": 41, "mask_last": 63, "mask_first_off": 64, "map_res_02": 13}
    assert c.dim[2] == want_z.get(name, 23)
    column = fits and c.dim[2] <= 32
    assert column == (name not in ("generic_33", "generic_41", "mask_last", "mask_first_off"))
    if name == "mixed_radius":
        assert len(set(c.radius)) > 1 and c.radius[0] == 0.15 and sum(r != c.radius[0] for r in c.radius) == 3
    if name == "far_origin":
        p = S.missions(name)[0].param
        assert (p.world_x_min, p.world_x_max, p.world_y_min, p.world_y_max) == (10.0, 14.0, -14.0, -10.0)
        assert np.spacing(np.float32(10.0)) > 0.9e-6   # a float32 ulp there is about the 1e-6 nudge


def test_grid_inside_world_has_faces_that_stop_at_the_grid():
    c = S.CASES["grid_inside_world"]
    stops = {"-x": 0, "+y": 0, "+z": 0}
    for s, (rc, ns, ref) in zip(S.missions(c.name), S.reference(c.name)):
        glo, ghi = S.grid_extent(s.world)
        p = s.param
        assert p.world_x_min == pytest.approx(glo[0] - 1.0) and p.world_y_max == pytest.approx(ghi[1] - c.res + 0.6) and \
            p.world_z_max == pytest.approx(ghi[2] - c.res + 0.8)
        for q in range(c.N):
            for b in ref.sfc_box[q, :ref.sfc_count[q]]:
                # the sample below a box that does not start at the world's edge lies at lo - 1e-6: the lowest face the grid allows is one cell in
                stops["-x"] += abs(b[0] - (glo[0] + c.res)) < 1e-9
                stops["+y"] += abs(b[4] - (ghi[1] - c.res)) < 1e-9
                stops["+z"] += abs(b[5] - (ghi[2] - c.res)) < 1e-9
                assert b[0] > p.world_x_min + 0.5 and b[4] < p.world_y_max - 0.3 and b[5] < p.world_z_max - 0.5   # never the world's edge
    assert all(v >= 1 for v in stops.values()), stops


def test_ties_025_has_seed_coordinates_on_exact_ties():
    c = S.CASES["ties_025"]
    ties = differ = zero_volume = 0
    for s in S.missions(c.name):
        t = s.plan.init_traj.astype(np.float64)
        for q in range(c.N):
            for i in range(c.M):
                lo = np.minimum(t[q, i], t[q, i + 1]) / 0.1
                hi = np.maximum(t[q, i], t[q, i + 1]) / 0.1
                for v in np.concatenate([lo, hi]):
                    if v - np.floor(v) == 0.5:
                        ties += 1
                        differ += S.c_round(v) != np.round(v)   # (half of the ties: numpy rounds them to even)
                sb = S.seed_box(s.plan.init_traj[q, i], s.plan.init_traj[q, i + 1], s.param)
                zero_volume += bool(np.all(sb[:3] == sb[3:]))
    assert ties >= 1 and differ >= 1 and zero_volume >= 1, (ties, differ, zero_volume)
    assert 0.25 / 0.1 == 2.5 and S.c_round(0.25 / 0.1) == 3.0 and np.round(0.25 / 0.1) == 2.0
