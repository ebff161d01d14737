"""The scene of the elevation grid: flat ground, a ramp of a known angle up to a plateau, a kerb of a known height, a wall
and a beam above the height band, seen from six sensor poses that drive up the ramp (pitched with it on the slope).  The
surfaces are sampled, not ray-cast: every scan holds the samples within range of its pose, in the sensor frame.  Used on
the reference alone in tests/test_elevation_host.py, which judges the layers by the masks on cell centres below."""
import functools
import math

import numpy as np

from tests import elevation_ref as E

RES = 0.25
GEO = E.geometry(resolution=RES, origin_x=-2.0, origin_y=-6.0, width=96, height=48, z_ref=0.0)
POINTS = E.point_params(z_lo=-2.5, z_hi=0.8, min_range=0.5, max_range=8.0)
LAYER = E.layer_params(min_points=3, window=2)
COST = E.cost_params(max_slope=0.35, max_step=0.25, max_rough=0.1, max_span=0.5)

RAMP_DEG = 10.0
RAMP_X0, RAMP_X1 = 8.0, 14.0
KERB_Y, KERB_H = 3.0, 0.15           # the ground is KERB_H higher for y > KERB_Y, on the flat before the ramp
WALL_Y, WALL_H = -5.0, 2.5
BEAM_X, BEAM_Z = 2.1, 2.2            # a bar across the track, above every pose's band
SENSOR_H = 1.0
POSE_X = (0.0, 3.0, 6.0, 9.0, 12.0, 15.0)
SPACING = 0.08


def ground(x, y):
    t = math.tan(math.radians(RAMP_DEG))
    z = np.clip(x - RAMP_X0, 0.0, RAMP_X1 - RAMP_X0) * t
    return z + np.where((y > KERB_Y) & (x < RAMP_X0), KERB_H, 0.0)


def surfaces():
    """the world's samples, (n, 3) float64: ground, wall, beam"""
    rng = np.random.default_rng(7)
    x0, y0 = GEO["origin_x"], GEO["origin_y"]
    xs = np.arange(x0 + 0.01, x0 + GEO["width"] * RES, SPACING)
    ys = np.arange(WALL_Y + 0.01, y0 + GEO["height"] * RES, SPACING)
    X, Y = (a.ravel() for a in np.meshgrid(xs, ys))
    X, Y = X + rng.uniform(0, 0.02, X.shape), Y + rng.uniform(0, 0.02, Y.shape)
    g = np.stack([X, Y, ground(X, Y)], 1)
    zs = np.arange(0.0, WALL_H, SPACING)
    Xw, Zw = (a.ravel() for a in np.meshgrid(xs, zs))
    wy = np.full_like(Xw, WALL_Y - 0.02)
    w = np.stack([Xw, wy, ground(Xw, wy) + Zw], 1)
    yb = np.arange(-4.0, 4.0, 0.02)
    b = np.stack([np.full_like(yb, BEAM_X), yb, np.full_like(yb, BEAM_Z)], 1)
    return np.concatenate([g, w, b])


def poses():
    """(6, 7) float64: a metre above the ground, pitched nose-up with the ramp where the pose stands on it"""
    out = []
    for x in POSE_X:
        on_ramp = RAMP_X0 < x < RAMP_X1
        half = 0.5 * math.radians(RAMP_DEG if on_ramp else 0.0)
        out.append([x, 0.0, float(ground(np.float64(x), np.float64(0.0))) + SENSOR_H, math.cos(half), 0.0, -math.sin(half), 0.0])
    return np.array(out, np.float64)


@functools.lru_cache(maxsize=None)
def scene():
    """dict(scans: list of (n, 3) float32 in the sensor frame, ids, poses)"""
    from tests import assemble_ref as A
    world, P = surfaces(), poses()
    scans = []
    for pose in P:
        near = np.linalg.norm(world - pose[:3], axis=1) < POINTS["max_range"] + 0.5
        R = A.rotation_matrix(pose)
        scans.append(((world[near] - pose[:3]) @ R).astype(np.float32))   # R^T (p - t)
    return dict(scans=scans, ids=np.arange(len(P)), poses=P)


@functools.lru_cache(maxsize=None)
def reference():
    """the definition on the scene, computed once: dict(cells, stats, layers, cost, summary) -- left unchanged by its users"""
    s = scene()
    ref = E.integrate(GEO, s["scans"], s["ids"], s["poses"], POINTS)
    assert not ref["error"]
    cost, summary, _ = E.cost(GEO, ref["cells"], LAYER, COST)
    return dict(cells=ref["cells"], stats=ref["stats"], layers=E.layers(GEO, ref["cells"], LAYER), cost=cost, summary=summary)


def centres():
    x = GEO["origin_x"] + (np.arange(GEO["width"]) + 0.5) * RES
    y = GEO["origin_y"] + (np.arange(GEO["height"]) + 0.5) * RES
    return np.meshgrid(x, y)


def measures():
    """the figures the scene is judged by"""
    ref = reference()
    L, cost = ref["layers"], ref["cost"]
    X, Y = centres()
    ramp = (X > RAMP_X0 + 3 * RES) & (X < RAMP_X1 - 3 * RES) & (np.abs(Y) < 2.5)
    flat = (X > 0.0) & (X < RAMP_X0 - 3 * RES) & (np.abs(Y) < 2.0)
    kerb = (np.abs(Y - KERB_Y) < RES) & (X > 0.0) & (X < RAMP_X0 - 3 * RES)         # the two rows that meet at the kerb
    wall = (np.abs(Y - (WALL_Y - 0.02)) < 0.5 * RES) & (X > 0.0) & (X < 16.0)
    beam = (np.abs(X - BEAM_X) < 0.5 * RES) & (np.abs(Y) < 2.0)
    tan = math.tan(math.radians(RAMP_DEG))
    return dict(ramp_cells=int(ramp.sum()), ramp_slope_median=float(np.median(L["slope"][ramp])),
                ramp_slope_worst=float(np.abs(L["slope"][ramp] - tan).max()), ramp_tan=tan,
                ramp_lethal=float((cost[ramp] == E.LETHAL).mean()), ramp_cost_median=float(np.median(cost[ramp])),
                flat_slope_max=float(L["slope"][flat].max()), flat_cost_max=int(cost[flat].max()),
                kerb_cells=int(kerb.sum()), kerb_step_median=float(np.median(L["step"][kerb])),
                kerb_step_worst=float(np.abs(L["step"][kerb] - KERB_H).max()), kerb_lethal=float((cost[kerb] == E.LETHAL).mean()),
                wall_cells=int(wall.sum()), wall_lethal=float((cost[wall] == E.LETHAL).mean()),
                beam_cells=int(beam.sum()), beam_max=float(L["max"][beam].max()), beam_lethal=float((cost[beam] == E.LETHAL).mean()))
