"""The six small kernels at the two ends of every estimate, entry by entry and at their edges -- k_tensorise_dlc, k_triangulate, k_project
(cpe_tensorise_dlc, cpe_triangulate, cpe_project_joints) on the ingestion side, k_fk, k_marker_vel, k_reproject (cpe_forward_kinematics,
cpe_marker_velocities, cpe_reproject) on the output side -- and the output arrays of k_finalize, against the longdouble / 40-digit
references of tests/ingest_compare.py.  tests/test_ingest_compare.py holds those references against the project's float64 routes on the same
cases (CPU).  Each case asserts that the path it means to exercise was taken and records its worst value per key; test_zz_report prints them.

Tolerances.  None comes from a kernel's output.  Every comparison is normalised by a scale stated at the assertion and held to
    MULT x gap + FLOOR x eps,     MULT = 8, FLOOR = 4, eps = 2.2e-16
where `gap` is the distance, on the very same case, between the reference and the project's float64 route (oracle.markers, com,
markers_jac @ dq, project, project_dependents, constraints, derivatives; initial_guess.triangulate_pixels with its float64 SVD), measured by
the functions of test_ingest_compare.py when the test runs.  The reason for 8 is at _ok().  The gather is compared bit for bit.

Gap of the float64 route | worst value of the kernel on an MI355X (test_zz_report; it fed no tolerance), in the normalisation of the assertion:
  k_fk           positions, of the base coordinate 1e3 m        2.3e-16 | 2.3e-16       centre of mass 1.0e-15 | 5.6e-16, its shift
                 with a massless link | 5.1e-16;  positions bit-equal with and without com
  k_marker_vel   of the largest marker speed                    2.6e-16 | 5.0e-16       one dof at a time, of the frame's speed | 3.0e-16
                 dq = 0 gives zeros, 2 dq exactly twice the bits
  k_reproject    of (|uv| + fx) kappa                           1.5e-16 | 6.1e-16 (theta = 1.4), 4.4e-17 at r <= 1e-3, on the axis the
                 principal point bit for bit, behind the camera 6.2e-17
  k_triangulate  of max(1, |xyz|): ring, exact pixels           5.6e-15 | 3.6e-15       1 px noise 1.3e-14 | 2.1e-14, monocular 1.2e-15 | 1.0e-15
                 baseline / depth 1, 0.3, 0.1                   8.9e-16, 4.0e-16, 1.1e-15 | 3.4e-16, 4.0e-16, 2.8e-16
                 0.03, 0.01, 3e-3                               3.6e-15, 5.6e-15, 4.2e-15 | 5.7e-16, 1.7e-15, 1.4e-14
                 1e-3, 5e-4 (0.05 m at 100 m)                   4.2e-14, 3.2e-14          | 5.9e-14, 2.8e-14
                 the same with 1 px noise                       1.6e-15 .. 7.1e-13        | 4.6e-16 .. 2.1e-13, each below its own gap x 4
                 outside the domain, against the 20-step checker | 5.6e-17
  k_project      of max(1, largest angle): scrambled +-0.3, +-3 2.1e-15, 1.5e-15 | 3.6e-15, 2.6e-15;  yaw moved by whole turns 4.1e-16 | 6.8e-16
                 equalities of the result (of the route's result 2.7e-15 at most) | 3.8e-15
                 |a_z / cos(theta)| = 1 - 1e-6, 1 - 1e-12       3.3e-14, 2.0e-11 | 1.8e-14, 4.6e-11;  the clamped frame 4.7e-16 | 1.8e-16
  k_finalize     dq, ddq of max|q| / h, 4 max|q| / h^2          4.9e-18, 1.4e-18 | 2.4e-17, (ddq below 1e-17);  dq0 = dq1 - h ddq1 | 9.2e-18
                 positions 1.7e-16 | 1.8e-16, meas_err of max|meas_err| + fx 2.7e-16 | 2.2e-16, equalities of the returned q | 4.4e-16
  k_tensorise_dlc  bit for bit in all 40 calls per size

What the file found (both repaired in the kernels, both shown by running this file on the library of the commit before):
  k_triangulate ran Jacobi on A^T A: 7.9e-14 against a gap of 5.6e-15 on the ring (record 14), 8.2e-13 against 1.3e-14 with noise, 1.3e-12
  against 3.2e-14 at baseline / depth 5e-4.  It now rotates the columns of A (one-sided Jacobi) and is within 3.5 x of the SVD route everywhere.
  k_project moved a calf's psi by whole turns towards its thigh's psi as it came in, not as projected: with dependent angles scrambled by
  +-3 rad, or the trunk's yaw moved by a turn, calves and hocks ended a whole turn from their parents.  cpe_project_joints also refused a
  null q before it looked at B N == 0.
"""
import numpy as np
import pytest

import ingest_compare as IC
import test_ingest_compare as TI
from cheetah_pose_estimation_amd import abi, skeleton, synth

pytestmark = pytest.mark.gpu

EPS = IC.EPS
MULT, FLOOR = 8, 4
WORST = {}
_HANDLES = {}


def _ok(key, err, gap, floor_scale=1.0):
    """records the worst normalised error of `key` and returns whether it is within MULT x gap + FLOOR x eps x floor_scale.
    MULT = 8: a kernel is one more float64 evaluation of the formula the route evaluates -- another order of operations, fused multiply-adds,
    another sin / cos -- so its distance from the reference is a draw from the distribution the route's distance is drawn from.  `gap` is the
    largest of the route's draws over the entries of the case; inside one case the route's own largest draw is up to 8 times its median
    (test_ingest_compare.py prints that spread for the triangulation, where it is widest), so 8 x gap is where a second evaluation as good as
    the route may land, and an evaluation that loses a digit does not.  FLOOR = 4 ulps of the scale stand in where the route happens to
    round exactly (gap 0)."""
    err = float(err)
    WORST[key] = max(WORST.get(key, 0.0), err)
    return err <= MULT * gap + FLOOR * EPS * floor_scale


def _handle(factory, key, sk, cams):
    if key not in _HANDLES:
        _HANDLES[key] = factory(sk, cams)
    return _HANDLES[key]


def _dev(a, dtype=np.float64):
    import torch
    return torch.tensor(np.ascontiguousarray(a, dtype=dtype), device=torch.device("cuda", 0))


def _full(shape, value=IC.SENTINEL):
    import torch
    return torch.full(tuple(shape), value, dtype=torch.float64, device=torch.device("cuda", 0))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------- cpe_forward_kinematics (k_fk)
def _fk(h, q, want_com):
    qd = _dev(q)
    pos = _full(q.shape[:2] + (h.L, 3))
    com = _full(q.shape[:2] + (3,)) if want_com else None
    h.forward_kinematics(qd, pos, com); h.synchronize()
    return pos.cpu().numpy(), None if com is None else com.cpu().numpy()


@pytest.mark.parametrize("name", IC.SKELETONS)
def test_forward_kinematics(name, gpu_handle_factory):
    """positions and centre of mass on every skeleton (the length-scaled one included: attach, marker_off and com all differ), angles out to
    +-3 pi, base a kilometre from the origin; com requested and not; the centre of mass also through a link whose mass is moved to zero"""
    sk = IC.model(name)
    h = _handle(gpu_handle_factory, ("fk", name), sk, synth.make_cameras(1))
    k = IC.massless_link(name)
    h0 = _handle(gpu_handle_factory, ("fk0", name), IC.without_mass(sk, k), synth.make_cameras(1))
    if name == "phantom25-scaled":
        plain = IC.model("phantom25")
        assert all(sk.attach[i][:] != plain.attach[i][:] for i in range(1, sk.n_links)) and sk.com[3][:] != plain.com[3][:]
        assert sum(sk.marker_off[l][:] != plain.marker_off[l][:] for l in range(24)) >= 20
    for shape in IC.SHAPES:
        c = TI.chain_case(name, shape)
        q, ref = c["q"], c["ref"]
        assert np.abs(q[..., 3:]).max() > 2.5 * np.pi and c["scale"] > 990 and q.shape[:2] == shape
        pos, com = _fk(h, q, True)
        pos_only, _ = _fk(h, q, False)
        assert _same_bits(pos, pos_only) and not (_bits(pos) == _bits(IC.SENTINEL)).any() and not (_bits(com) == _bits(IC.SENTINEL)).any()
        # scale: the largest base coordinate of the case (1e3 m)
        assert _ok(f"fk pos {name}", IC.worst(pos, ref["pos"], c["scale"]), c["gap"]["pos"]), (name, shape)
        assert _ok(f"fk com {name}", IC.worst(com, ref["com"], c["scale"]), c["gap"]["com"]), (name, shape)
        # second route: the shift of the centre of mass when link k weighs nothing, m_k (com - centre_k) / (M - m_k) by the reference.  Two
        # kernel results enter the difference, each with the tolerance above
        _, com0 = _fk(h0, q, True)
        m = IC.ld([sk.mass[i] for i in range(sk.n_links)])
        want = m[k] * (ref["com"] - ref["centre"][..., k, :]) / (m.sum() - m[k])
        assert np.abs(np.asarray(want, dtype=np.float64)).max() > 1e-4      # 0.1 mm and more: nine digits above eps x 1e3 m
        e = IC.worst(IC.ld(com0) - IC.ld(com), want, c["scale"])
        WORST[f"fk com shift {name}"] = max(WORST.get(f"fk com shift {name}", 0.0), e)
        assert e <= 2 * (MULT * c["gap"]["com"] + FLOOR * EPS), (name, shape, e)


# ---------------------------------------------------------------------------------------------------- cpe_marker_velocities (k_marker_vel)
def _vel(h, q, dq):
    vel = _full(q.shape[:2] + (h.L, 3))
    h.marker_velocities(_dev(q), _dev(dq), vel); h.synchronize()
    return vel.cpu().numpy()


@pytest.mark.parametrize("name", IC.SKELETONS)
def test_marker_velocities(name, gpu_handle_factory):
    """(d p / d q) dq against the forward-mode reference and against oracle.markers_jac @ dq; exactly zero for dq = 0, exactly doubled for 2 dq"""
    sk = IC.model(name)
    h = _handle(gpu_handle_factory, ("fk", name), sk, synth.make_cameras(1))
    for shape in IC.SHAPES:
        c = TI.chain_case(name, shape)
        vel = _vel(h, c["q"], c["dq"])
        # scale: the largest marker speed of the case
        assert _ok(f"vel {name}", IC.worst(vel, c["ref"]["vel"], c["vscale"]), c["gap"]["vel"]), (name, shape)
        assert IC.worst(vel, c["route"]["vel"], c["vscale"]) <= (MULT + 1) * c["gap"]["vel"] + FLOOR * EPS      # the route itself: one gap further at most
        assert (_bits(_vel(h, c["q"], np.zeros_like(c["dq"]))) << 1 == 0).all()                              # +-0 and nothing else
        assert _same_bits(_vel(h, c["q"], 2.0 * c["dq"]), 2.0 * vel)


def test_marker_velocity_columns(gpu_handle_factory):
    """one non-zero rate per frame, swept over all 54 dofs: a wrong slot_dof shows as a wrong column"""
    name = "phantom25-scaled"
    sk = IC.model(name)
    h = _handle(gpu_handle_factory, ("fk", name), sk, synth.make_cameras(1))
    seen = []
    for q, dq in IC.dof_sweep(name):
        assert ((dq != 0).sum(axis=-1) == 1).all()
        seen += list(np.nonzero(dq.reshape(-1, sk.nq))[1])
        ref = IC.chain(sk, q, dq)["vel"]
        route = np.stack([TI.O.markers_jac(sk, x)[1] @ v for x, v in zip(q.reshape(-1, sk.nq), dq.reshape(-1, sk.nq))]).reshape(ref.shape)
        vscale = float(np.abs(np.asarray(ref, dtype=np.float64)).max())
        vel = _vel(h, q, dq)
        # per frame, so that a column that is small beside the largest one still counts: scale = the frame's own largest speed.  (The roll of
        # a link whose markers lie on its own x axis moves nothing: that frame is all zeros, exactly, below.)
        fscale = np.abs(np.asarray(ref, dtype=np.float64)).max(axis=(-1, -2), keepdims=True)
        assert (fscale > 1e-3).sum() >= 24
        fscale[fscale == 0] = 1.0
        gap = IC.worst(ref, route, fscale)
        assert _ok("vel single dof", IC.worst(vel, ref, fscale), gap) and vscale > 0
        assert (vel[np.asarray(ref, dtype=np.float64) == 0] == 0).all()          # markers the dof does not move stay exactly still
    assert sorted(seen) == list(range(54))


# ---------------------------------------------------------------------------------------------------- cpe_reproject (k_reproject)
@pytest.mark.parametrize("L", [24, 25])
@pytest.mark.parametrize("C", IC.REPROJECT_CAMS)
def test_reproject(C, L, gpu_handle_factory):
    """C L = 24 .. 450 (camera, marker) pairs: less than one stride of 64 up to eight; both camera models in one handle; points on the optical
    axis, at r = 1e-12 .. 1e-3 from it, out to theta = 1.4 and behind the camera; every entry of the sentinel-filled output written"""
    c = TI.camera_case(C, L)
    h = _handle(gpu_handle_factory, ("reproject", C, L), skeleton.build_skeleton("phantom", L), c["cams"])
    assert h.n_cams == C and h.L == L and {cam.model for cam in c["cams"]} == ({abi.CAM_FISHEYE, abi.CAM_PINHOLE} if C > 1 else {abi.CAM_FISHEYE})
    uv = _full((2, 5, C, L, 2))
    h.reproject(_dev(c["pos"]), uv); h.synchronize()
    uv = uv.cpu().numpy()
    assert not (_bits(uv) == _bits(IC.SENTINEL)).any()                 # the last frame and the last camera included
    assert c["finite"].all() and np.isfinite(uv).all()
    # scale per entry: (|uv| + fx) kappa, kappa = (|R2| . |p| + |t2|) / |X2| the cancellation in the depth (test_ingest_compare.camera_case)
    err = np.asarray(np.abs(IC.ld(uv) - c["ref"]) / c["scale"], dtype=np.float64)
    k = c["kinds"]
    for kind, sl in list(k.items()) + [("markers", None)]:
        e = err[0, 0, :, sl].max() if sl is not None else err[:, 1:4].max()
        WORST[f"reproject {kind}"] = max(WORST.get(f"reproject {kind}", 0.0), float(e))
    assert _ok(f"reproject C = {C}", err.max(), c["gap"]), (C, L, np.unravel_index(err.argmax(), err.shape))
    # a point on the axis lands on the principal point exactly (0 x anything / 1e-12 = 0)
    for cam_i in range(min(C, 2)):
        assert (uv[0, 0, cam_i, k["axis"]] == [c["cams"][cam_i].cx, c["cams"][cam_i].cy]).all()
    assert _same_bits(uv[0, 0], uv[1, 4])                              # the edge frame again as the last frame of the batch


# ---------------------------------------------------------------------------------------------------- cpe_triangulate (k_triangulate)
TRI_MARGIN = 8      # the measured spread of the float64 SVD route: inside one geometry class its largest error is up to 8 x its median
#                     (test_ingest_compare.test_triangulation_reference prints it; one class, baseline / depth 5e-4 with noise, has a single
#                     record at 200 x, which only widens that class's own gap).  Same number as MULT, for the same reason.


def _tri_handle(factory, which):
    r = TI.tri_case(which)["rec"]
    return _handle(factory, ("tri", which), skeleton.build_skeleton("phantom", 24), r["cams"])


def _tri_check(which, got, n, label):
    """got [n, 3] against the 40-digit reference, class by class: scale max(1, |xyz|) per record; the floor carries 1 / cos^2(theta) of the
    record's widest fisheye ray (tan amplifies the last bit of theta by that: 200 at theta = 1.5)"""
    c = TI.tri_case(which)
    ex = c["exact"]
    err = np.asarray(np.abs(IC.ld(got) - ex["xyz"][:n]).max(axis=1), dtype=np.float64) / c["scale"][:n]
    bad = {}
    for case, idx in TI.tri_cases(which).items():
        idx = idx[idx < n]
        for i in idx:
            if not _ok(f"{label} {case}", err[i], c["gap"][case], 1.0 / np.cos(ex["theta"][i]) ** 2):
                bad[(case, int(i))] = (err[i], c["gap"][case])
    return bad


@pytest.mark.parametrize("n", IC.TRI_SIZES)
def test_triangulate_sizes(n, gpu_handle_factory):
    """n at and around the 256-lane block edge; two-view and monocular lanes and both camera models inside every run of four lanes; all 30
    ordered camera pairs; exact float64 projections and 1 px noise; a pixel exactly on the principal point (the rd <= 1e-12 branch)"""
    assert MULT == TRI_MARGIN
    h = _tri_handle(gpu_handle_factory, "rig")
    r = TI.tri_case("rig")["rec"]
    got = h.triangulate_host(r["cam_a"][:n], r["cam_b"][:n], r["uv_a"][:n], r["uv_b"][:n], depth=IC.TRI_DEPTH)
    assert got.shape == (n, 3) and (n + 255) // 256 == {1: 1, 255: 1, 256: 1, 257: 2, 513: 3}[n]
    if n >= 255:
        two = r["cam_b"][:64] >= 0                                    # the first wave holds all four branches
        fish = np.array([r["cams"][int(a)].model == abi.CAM_FISHEYE for a in r["cam_a"][:64]])
        assert all((two == t).__and__(fish == f).any() for t in (True, False) for f in (True, False))
        assert r["cam_b"][7] < 0 and r["cam_a"][8] == 4               # the principal-point records are in
    bad = _tri_check("rig", got, n, "triangulate")
    assert not bad, (n, bad)


def test_triangulate_baselines(gpu_handle_factory):
    """baseline / depth from 1 down to 5e-4 (0.05 m at 100 m), exact projections and 1 px noise, against the float64 SVD route's own distance
    from 40 digits.  Jacobi on A^T A failed this from 0.03 down (3.6 digits lost at 1e-3); the kernel now rotates the columns of A itself."""
    h = _tri_handle(gpu_handle_factory, "baseline")
    r = TI.tri_case("baseline")["rec"]
    got = h.triangulate_host(r["cam_a"], r["cam_b"], r["uv_a"], r["uv_b"], depth=IC.TRI_DEPTH)
    assert len(r["cam_a"]) == 64 and (r["cam_b"] >= 0).all()
    bad = _tri_check("baseline", got, 64, "triangulate")
    assert not bad, bad


def test_triangulate_outside_the_undistortion_domain(gpu_handle_factory):
    """the one case outside the domain (pinhole k1 = -0.3, r = 0.7: contraction 0.34): 20 fixed-point steps stop 2e-11 short of the exact
    inverse, so this record is compared with the 20-step checker only, which takes the same steps: 16 ulps of max(1, |xyz|) (a contraction by
    0.34 forgets the rounding of earlier steps; what is left is the last steps' and the back-projection's)"""
    c = TI.tri_case("outside")
    r = c["rec"]
    h = _tri_handle(gpu_handle_factory, "outside")
    got = h.triangulate_host(r["cam_a"], r["cam_b"], r["uv_a"], r["uv_b"], depth=IC.TRI_DEPTH)
    assert c["exact"]["contraction"][0] > IC.CONTRACTION_MAX and c["err"][0] > 1e3 * EPS
    e = IC.worst(got, c["route"], c["scale"][:, None])
    WORST["triangulate outside domain vs 20-step checker"] = e
    assert e <= 16 * EPS


def test_triangulate_edges_of_the_call(gpu_handle_factory):
    """n = 0 with null arrays is OK; a camera index out of range in the last of 257 records is refused and xyz is left alone"""
    h = _tri_handle(gpu_handle_factory, "rig")
    r = TI.tri_case("rig")["rec"]
    assert h.lib.cpe_triangulate(h._h, 0, None, None, None, None, 3.0, None) == abi.OK
    n = 257
    for bad_a, bad_b in ((6, 0), (0, 6), (-1, 0)):
        ca, cb = r["cam_a"][:n].copy(), r["cam_b"][:n].copy()
        ca[-1], cb[-1] = bad_a, bad_b
        xyz = _full((n, 3))
        d = [_dev(ca, np.int32), _dev(cb, np.int32), _dev(r["uv_a"][:n]), _dev(r["uv_b"][:n])]
        st = h._call(h.lib.cpe_triangulate, "cpe_triangulate", n, *[t.data_ptr() for t in d], 3.0, xyz.data_ptr(), allow=(abi.OK, abi.BAD_ARG))
        h.synchronize()
        assert st == abi.BAD_ARG and b"camera index" in h.lib.cpe_last_error()
        assert (_bits(xyz.cpu().numpy()) == _bits(IC.SENTINEL)).all()


# ---------------------------------------------------------------------------------------------------- cpe_tensorise_dlc (k_tensorise_dlc)
@pytest.mark.parametrize("L,N", IC.DLC_SIZES)
def test_tensorise_dlc(L, N, gpu_handle_factory):
    """called directly: N L = 24, 600, 768 (three full blocks of 256), 775; first_row before, at, near the end of, at the end of and past the
    table; likelihood at, one ulp above and one ulp below the threshold, NaN, +-inf; x or y NaN, +-inf; body parts -1 and `parts`; one slot,
    and slots 5, 0, 3 of six.  Bit for bit against the numpy rule on sentinel-filled arrays: what the call does not own stays the sentinel."""
    h = _handle(gpu_handle_factory, ("dlc", L), skeleton.build_skeleton("phantom", L), synth.make_cameras(1))
    t, pm, isg, where = IC.dlc_inputs(L)
    assert N * L == {(24, 1): 24, (24, 25): 600, (24, 32): 768, (25, 31): 775}[(L, N)] and (pm == -1).sum() == 1 and (pm == IC.DLC_PARTS).sum() == 1
    td, pmd, isgd = _dev(t), _dev(pm, np.int32), _dev(isg)
    read = set()
    for first_row in IC.dlc_first_rows():
        for n_slots, slots in ((1, (0,)), (6, (5, 0, 3))):
            meas, weight = _full((N, n_slots, L, 2)), _full((N, n_slots, L))
            for s in slots:
                h._call(h.lib.cpe_tensorise_dlc, "cpe_tensorise_dlc", N, n_slots, s, td.data_ptr(), IC.DLC_ROWS, IC.DLC_PARTS, first_row, pmd.data_ptr(),
                        isgd.data_ptr(), IC.DLC_THRESH, meas.data_ptr(), weight.data_ptr())
            h.synchronize()
            want_m, want_w = TI.dlc_expected(L, N, n_slots, slots, first_row)
            gm, gw = meas.cpu().numpy(), weight.cpu().numpy()
            assert _same_bits(gm, want_m) and _same_bits(gw, want_w), (first_row, n_slots)
            untouched = [s for s in range(n_slots) if s not in slots]
            assert (_bits(gw[:, untouched]) == _bits(IC.SENTINEL)).all() and not (_bits(gw[:, list(slots)]) == _bits(IC.SENTINEL)).any()
            inside = (0 <= first_row + np.arange(N)) & (first_row + np.arange(N) < IC.DLC_ROWS)
            assert (gw[~inside][:, list(slots)] == 0).all() and ((gw[inside][:, list(slots)] > 0).any() or not inside.any())
            read |= {(row, part) for row, part in where if 0 <= row - first_row < N and part in pm}
    assert len(where) == 36 and (len(read) == 36 or N == 1)            # every special entry went through the kernel (one frame reaches a few)


# ---------------------------------------------------------------------------------------------------- cpe_project_joints (k_project)
def _project(h, q):
    qd = _dev(q)
    st = h.project_joints(qd)
    return st, qd.cpu().numpy()


def _joints_ok(label, c, got, floor_scale=1.0):
    """dependent angles against the closed form (scale: max(1, largest angle)), the 26 equalities of the result in longdouble against those of
    the route's result, independent angles bit for bit"""
    sk = c["sk"]
    ind = skeleton.independent_dofs(sk)
    assert _same_bits(got[..., ind], c["q"][..., ind]), label
    ok = _ok(f"project q {label}", IC.worst(got, c["ref"]["q"], c["scale"]), c["gap"]["q"], floor_scale)
    return ok and _ok(f"project equalities {label}", np.abs(IC.joint_equalities(sk, got)).max(), c["gap"]["eq_of_route"], floor_scale)


@pytest.mark.parametrize("name", IC.PROJECT_MODELS)
def test_project_joints(name, gpu_handle_factory):
    """dependent angles scrambled by +-0.3 and +-3 rad, and the trunk's yaw moved by 0, +-1, +-3 and 3.5 turns with the legs' yaw left behind:
    every child's psi follows its parent's by whole turns -- the calf's follows the thigh's NEW psi, two and three links down the chain"""
    sk = IC.model(name)
    h = _handle(gpu_handle_factory, ("project", name), sk, synth.make_cameras(1))
    rev = [j for j in range(sk.n_joints) if sk.joint_kind[j] == abi.JOINT_REVOLUTE_Y]
    par, chi = [3 + 3 * sk.joint_parent[j] + 2 for j in rev], [3 + 3 * sk.joint_child[j] + 2 for j in rev]
    for kind, value in TI.JOINT_CASES[:-len(IC.EDGE_RATIOS)]:
        c = TI.joints_case(name, kind, value)
        st, got = _project(h, c["q"])
        assert st == abi.OK and not c["ref"]["clamped"].any()
        if kind == "yaw" and value != 0:
            moved = c["ref"]["turns"][..., rev] - TI.joints_case(name, "yaw", 0.0)["ref"]["turns"][..., rev]
            assert (moved != 0).all()                                  # the wrap count is non-zero in every joint of every frame
        if kind == "scramble" and value == 3.0:
            # children whose parent's psi came in more than half a turn from where the child's ends up: turns taken towards that stale
            # value would leave the child a whole turn from the reference
            stale = np.abs(c["q"][..., par] - np.asarray(c["ref"]["q"][..., chi], dtype=np.float64)) > np.pi
            assert stale.sum() > 20
        assert np.abs(got[..., chi] - got[..., par]).max() < np.pi, (kind, value)
        assert _joints_ok(f"{kind} {value:.3g}", c, got), (name, kind, value)


@pytest.mark.parametrize("name", IC.PROJECT_MODELS)
def test_project_joints_gimbal_band(name, gpu_handle_factory):
    """|a_z / cos(theta)| at 1 - 1e-6, 1 - 1e-12 and 1 + 1e-3: below the edge the call is OK and phi is held to the tolerance over cos(phi);
    above it the call returns CPE_NUMERICAL, the clamped frame holds the clamped closed form, every other frame of the batch is bit-equal to
    its result without the clamped frame, and the next clean call on the handle returns CPE_OK"""
    sk = IC.model(name)
    h = _handle(gpu_handle_factory, ("project", name), sk, synth.make_cameras(1))
    for ratio in IC.EDGE_RATIOS[:2]:
        c = TI.joints_case(name, "gimbal", ratio)
        st, got = _project(h, c["q"])
        assert st == abi.OK and not c["ref"]["clamped"].any() and abs(c["ref"]["ratio"].max() / ratio - 1) < 1e-9
        assert _joints_ok(f"edge {1 - ratio:.0e} below", c, got, 1.0 / np.sqrt(1 - min(ratio, 1 - EPS) ** 2)), (name, ratio)
    c = TI.joints_case(name, "gimbal", IC.EDGE_RATIOS[2])
    batch = TI.joints_case(name, "scramble", 0.3)
    assert c["ref"]["clamped"].all() and c["ref"]["ratio"].max() > 1 and batch["q"].shape[:2] == (3, 16)
    st_clean, clean = _project(h, batch["q"])
    assert st_clean == abi.OK
    for b, n in ((1, 7), (2, 15)):                                     # in the middle of the batch, and as its very last frame
        q = batch["q"].copy()
        q[b, n] = c["q"][0, 0]
        st, got = _project(h, q)
        assert st == abi.NUMERICAL, (b, n)
        others = np.ones((3, 16), bool); others[b, n] = False
        assert _same_bits(got[others], clean[others])
        # the clamped frame: sin(phi) = +-1 exactly, phi = +-pi / 2, psi by the same formula (scale: max(1, largest angle))
        ind = skeleton.independent_dofs(sk)
        assert _same_bits(got[b, n, ind], q[b, n, ind])
        assert _ok("project q clamped frame", IC.worst(got[b, n], c["ref"]["q"][0, 0], c["scale"]), c["gap"]["q"]), (name, b, n)
        st_again, again = _project(h, batch["q"])                     # the flag of the handle is reset between calls
        assert st_again == abi.OK and _same_bits(again, clean)
    # an empty call takes a null q, as its neighbours do; a call with frames does not
    assert h.lib.cpe_project_joints(h._h, 0, 5, None) == abi.OK and h.lib.cpe_project_joints(h._h, 3, 0, None) == abi.OK
    assert h.lib.cpe_project_joints(h._h, 1, 1, None) == abi.BAD_ARG and b"null" in h.lib.cpe_last_error()


# ---------------------------------------------------------------------------------------------------- outputs of a solve (k_finalize)
@pytest.mark.parametrize("N", [1, 2, 3, 4, 9])
def test_solve_outputs_follow_from_the_returned_q(N, gpu_handle_factory):
    """cpe_solve_host, stopped after three iterations (k_finalize writes the outputs whatever the status): dq, ddq, positions and meas_err
    recomputed in longdouble from the returned q and the call's inputs alone -- the gauge ddq0 = ddq1 = ddq2, dq0 = dq1 - h ddq1, the zeros
    of short sequences, zero-weight measurements -- and the joint equalities of the returned q"""
    sk, cams = IC.model("phantom25"), synth.make_cameras(6)
    opts = abi.default_options()
    opts.max_iter = 3
    if "solve" not in _HANDLES:
        _HANDLES["solve"] = gpu_handle_factory(sk, cams, opts)
    h = _HANDLES["solve"]
    d = synth.make_batch(sk, cams, B=2, N=N, seed=60 + N)
    meas, weight = d["meas"].copy(), d["weight"].copy()
    weight[:, :, 1::2, 3] = 0.0
    meas[weight == 0] = 0.0
    assert (weight == 0).sum() > 10 and (weight > 0).sum() > 10
    out = h.solve_host(d["q_init"], meas, weight)
    hh = opts.h
    for b in range(2):
        q = out["q"][b]
        ref, gap, scale = TI.outputs_gap(sk, cams, hh, q, meas[b])
        for key in ("dq", "ddq", "positions", "meas_err"):
            # scales: max|q| / h, 4 max|q| / h^2, max|q|, max|meas_err| + fx
            assert _ok(f"finalize {key}", IC.worst(out[key][b], ref[key], scale[key]), gap[key]), (N, b, key)
        dq, ddq = out["dq"][b], out["ddq"][b]
        if N < 3:
            assert (_bits(ddq) == 0).all()
        else:
            assert _same_bits(ddq[0], ddq[2]) and _same_bits(ddq[1], ddq[2]) and np.abs(ddq[2]).max() > 0
        if N == 1:
            assert (_bits(dq) == 0).all()
        else:
            e = IC.worst(dq[0], IC.ld(dq[1]) - IC.LD(hh) * IC.ld(ddq[1]), scale["dq"])
            assert _ok("finalize dq0 = dq1 - h ddq1", e, 0.0) and np.abs(dq[1]).max() > 0
        route_q = TI.O.project_dependents(sk, q)
        assert _ok("finalize equalities of q", np.abs(IC.joint_equalities(sk, q)).max(), float(np.abs(IC.joint_equalities(sk, route_q)).max())), (N, b)


def test_zz_report():
    """the worst normalised value of every comparison of this module (shown with -s); the figures of the module's docstring"""
    for k in sorted(WORST):
        print(f"  {k}: {WORST[k]:.1e}")
