"""References and case tables for the scene encoders' kernels (scene.hip) at ragged and edge shapes (numpy / torch on the CPU, no GPU).

The three stages that look across tokens, each with a float64 restatement (the truth) and a plain float32 evaluation on the CPU (the
yardstick of the bars; neither shares code with the kernels):

  attention   qkv (T, 3 E) = [q | k | v], E = 4 dh, head h at column h dh; o (T, E) = softmax(dh^-0.5 q k^T) v per head
  colreduce   x (rows, C), segment s = rows [first[s], first[s + 1]) -> mean or max per column
  prep        cloud (No, Np, 2) -> centre of each obstacle and its largest |coordinate - centre|

and the clouds / state dicts of the whole-encoder ("latent") cases, measured against oracle.ramp_oracle's float64 encoders.

Bars: attention_ref.bar(b0, floor) = max(b0, 4 floor) with b0 the project's existing bar (latents 5e-6, attention B0["attention"]);
column reduce and prep have no existing bar, theirs is 4 max(floor, ULP_FLOOR).  `floor` is the float32 evaluation's error against
float64 in the same metric; no bar is ever derived from a kernel's output.

The float32 yardstick of the column MEAN adds the rows one after the other: the error of a float32 sum depends on its order, and a
pairwise sum (numpy's, torch's) is a different algorithm with a smaller error than any serial single-precision sum -- the same choice
attention_ref makes for its logits.  The prep metric divides by the largest |coordinate|, for maxd too: maxd is a difference of
coordinates and inherits the centre's rounding error, which lives on the coordinate scale, not on maxd's own (smaller) one."""
from collections import OrderedDict

import numpy as np
import torch

from ramp_amd import synth
from attention_ref import B0, FLOOR_CAP, bar, rel        # noqa: F401  (re-exported: the tests take the rule and the metric from here)
from util import weights

HEADS = 4
DHS = (16, 64)
TILE = 64                                            # queries of one attention block, keys of one LDS tile
LENGTHS = [1, 2, 63, 64, 65, 128, 129, 200]
REGIMES = ["gauss", "sharp", "late_max", "early_max", "onehot_across_tiles", "equal_large", "flat", "zero_v"]
RAGGED = [7, 150, 64, 1, 65]                         # scene lengths of the segmented form
SHARP_MEAN_MAX_P = 0.9                               # lower bound of the mean over queries of max_k P, at T >= 16
LATENT_B0 = 5e-6                                     # the project's latent bar (against the reference's fixtures)
LATENT_F32_CAP = 2.5e-6                              # rel(oracle float32, oracle float64) of every latent case: half the bar
ULP_FLOOR = 2.0 * 2.0 ** -23                         # two float32 ulps of the output scale: the floor of an exactly computed case


def stage_bar(floor):
    """Column reduce and prep: 4 x the float32 evaluation's error, and never below 4 x two ulps."""
    return 4.0 * max(floor, ULP_FLOOR)


# ---- attention ----------------------------------------------------------------------------------------------------------------------
def lengths_of(regime):
    """A winning key in ANOTHER 64-key tile needs more than one tile."""
    return [T for T in LENGTHS if T > TILE] if regime == "onehot_across_tiles" else LENGTHS


def onehot_target(T):
    """Key every query of onehot_across_tiles points at: the same offset in the next tile (cyclically), folded into a short last tile."""
    nt = (T + TILE - 1) // TILE
    i = np.arange(T)
    tt = (i // TILE + 1) % nt
    size = np.minimum(TILE, T - tt * TILE)
    return tt * TILE + (i % TILE) % size


def make_attention_case(regime, T, dh):
    """qkv (T, 3 E) float32."""
    assert regime in REGIMES and dh in DHS
    g = np.random.Generator(np.random.PCG64([1009 * REGIMES.index(regime) + 31 * T + dh, 23]))
    E = HEADS * dh
    q = g.standard_normal((T, HEADS, dh)); k = g.standard_normal((T, HEADS, dh))
    v = g.standard_normal((T, HEADS, dh)) * 0.4 + 0.1
    if regime == "sharp":
        q *= 6.0; k *= 6.0
    elif regime in ("late_max", "early_max"):
        # k_j = a_j u, q_i = c_i u + (a part orthogonal to u): logit(i, j) = c_i a_j |u|^2 / sqrt(dh) = 0.25 c_i rank(j), c_i in [1, 2]
        u = g.integers(0, 2, size=(HEADS, dh)) * 2.0 - 1.0
        rank = np.arange(T) if regime == "late_max" else np.arange(T)[::-1]
        k = (0.25 * rank / np.sqrt(dh))[:, None, None] * u[None]
        c = 1.0 + g.random((T, HEADS, 1))
        q = q - (q * u).sum(-1, keepdims=True) / dh * u
        q = q + c * u
    elif regime == "onehot_across_tiles":
        assert T > TILE
        k *= np.sqrt(dh) / np.linalg.norm(k, axis=-1, keepdims=True)        # equal norms: k_t . k_j < |k|^2 for every j != t
        q = 8.0 * k[onehot_target(T)]
    elif regime == "equal_large":
        k = np.repeat(g.standard_normal((1, HEADS, dh)), T, axis=0)         # one key for all: a query's logits are equal in any arithmetic
        q = (1.0 + 0.05 * g.standard_normal((T, HEADS, 1))) * k * (60.0 * np.sqrt(dh) / (k * k).sum(-1, keepdims=True))
    elif regime == "flat":
        q[:] = 0.0
    elif regime == "zero_v":
        q *= 1.3; k *= 1.3; v[:] = 0.0
    return np.concatenate([q.reshape(T, E), k.reshape(T, E), v.reshape(T, E)], axis=1).astype(np.float32)


def _heads(qkv, dh):
    T = qkv.shape[0]
    x = np.asarray(qkv).reshape(T, 3, HEADS, dh)
    return x[:, 0].transpose(1, 0, 2), x[:, 1].transpose(1, 0, 2), x[:, 2].transpose(1, 0, 2)      # each (4, T, dh)


def logits_ref64(qkv, dh):
    q, k, _ = _heads(np.asarray(qkv, np.float64), dh)
    return (q @ k.transpose(0, 2, 1)) * dh ** -0.5


def probs_ref64(qkv, dh):
    """P (4, T, T) in float64, the row maximum subtracted."""
    s = logits_ref64(qkv, dh)
    e = np.exp(s - s.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def attn_ref64(qkv, dh):
    """o (T, E), float64."""
    v = _heads(np.asarray(qkv, np.float64), dh)[2]
    return (probs_ref64(qkv, dh) @ v).transpose(1, 0, 2).reshape(qkv.shape[0], HEADS * dh)


def attn_fp32(qkv, dh):
    """The same in float32 with torch on the CPU (logits through a plain float32 matrix product)."""
    T = qkv.shape[0]
    x = torch.from_numpy(np.ascontiguousarray(qkv, dtype=np.float32)).reshape(T, 3, HEADS, dh)
    q, k, v = x[:, 0].transpose(0, 1), x[:, 1].transpose(0, 1), x[:, 2].transpose(0, 1)
    p = torch.softmax(q @ k.transpose(-1, -2) * np.float32(dh ** -0.5), dim=-1)
    return (p @ v).transpose(0, 1).reshape(T, HEADS * dh).numpy()


_ATT = {}


def attention_case(regime, T, dh):
    """Inputs, float64 reference, float32 evaluation and its error, computed once per process and left unchanged."""
    key = (regime, T, dh)
    if key not in _ATT:
        qkv = make_attention_case(regime, T, dh)
        o64, o32 = attn_ref64(qkv, dh), attn_fp32(qkv, dh)
        for a in (qkv, o64, o32):
            a.setflags(write=False)
        _ATT[key] = dict(regime=regime, T=T, dh=dh, qkv=qkv, o=o64, o32=o32, floor=rel(o32, o64))
    return _ATT[key]


def attention_tiles(lengths):
    """tiles (n_tiles, 3) int32 as ramp_encode_scenes builds them: {scene's first row, scene's row count, first query} per 64 queries."""
    out, base = [], 0
    for Ts in lengths:
        out += [(base, Ts, q0) for q0 in range(0, Ts, TILE)]
        base += Ts
    return np.asarray(out, dtype=np.int32)


def ragged_attention_case(regime, dh):
    """The scenes of RAGGED, each a case of its own length, row after row: (qkv, [per-scene case])."""
    parts = [attention_case(regime, T, dh) for T in RAGGED]
    return np.concatenate([p["qkv"] for p in parts]), parts


# ---- column reduce ------------------------------------------------------------------------------------------------------------------
COLREDUCE_SWEEP = [(seglen, C, n_seg) for seglen in (1, 2, 63, 64, 65, 1000) for C in (64, 256) for n_seg in (1, 3)]
COLREDUCE_RAGGED = [1, 65, 2, 1000, 64]              # segment lengths of the segmented form


def make_colreduce_case(kind, rows, C, seed):
    """x (rows, C) float32: "gauss", "negative" (every entry below -0.5) or "ties" (multiples of 0.5 in [-1.5, 1]: every column's
    maximum occurs many times once a segment has a few dozen rows)."""
    g = np.random.Generator(np.random.PCG64([seed, 29]))
    if kind == "gauss":
        x = g.standard_normal((rows, C)) + 0.25
    elif kind == "negative":
        x = -(np.abs(g.standard_normal((rows, C))) + 0.5)
    else:
        assert kind == "ties"
        x = np.minimum(g.integers(-3, 7, size=(rows, C)), 2) * 0.5          # half of the entries sit at the top value 1
    return x.astype(np.float32)


def csr(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)


def colreduce_ref64(x, first, mode):
    """out (n_seg, C) float64: mode 0 the mean, 1 the maximum over the rows [first[s], first[s + 1])."""
    x = np.asarray(x, np.float64)
    f = (lambda a: a.max(0)) if mode else (lambda a: a.mean(0))
    return np.stack([f(x[first[s]:first[s + 1]]) for s in range(len(first) - 1)])


def colreduce_fp32(x, first, mode):
    """The same in float32; the mean adds the rows serially (see the module docstring)."""
    x = np.asarray(x, np.float32)
    out = np.empty((len(first) - 1, x.shape[1]), np.float32)
    for s in range(len(first) - 1):
        seg = x[first[s]:first[s + 1]]
        if mode:
            out[s] = seg.max(0)
        else:
            acc = np.zeros(x.shape[1], np.float32)
            for row in seg:
                acc = acc + row
            out[s] = acc / np.float32(len(seg))
    return out


# ---- prep ---------------------------------------------------------------------------------------------------------------------------
PREP_SWEEP = [(No, Np) for Np in (1, 2, 63, 64, 65, 130) for No in (1, 5)]
IDENTICAL_EXACT = np.tile(np.array([0.375, -0.625], np.float32), (1, 16, 1))        # multiples of 1/8: float32 sum and mean are exact
IDENTICAL_INEXACT_POINT = (0.1, 0.7)                 # not representable: the float32 mean is an ulp off the point (excluded from accuracy)


def make_prep_case(No, Np):
    g = np.random.Generator(np.random.PCG64([131 * No + Np, 31]))
    centre = g.uniform(-0.7, 0.7, size=(No, 1, 2))
    return (centre + g.uniform(-0.13, 0.13, size=(No, Np, 2))).astype(np.float32)


def prep_ref64(cloud):
    """(centres (No, 2), maxd (No)) in float64."""
    x = np.asarray(cloud, np.float64)
    c = x.mean(1)
    return c, np.abs(x - c[:, None]).reshape(x.shape[0], -1).max(-1)


def prep_fp32(cloud):
    x = np.asarray(cloud, np.float32)
    c = x.sum(1, dtype=np.float32) / np.float32(x.shape[1])
    return c, np.abs(x - c[:, None]).reshape(x.shape[0], -1).max(-1)


def prep_errors(got, ref, cloud):
    """(centre error, maxd error), both over the largest |coordinate| of the cloud."""
    scale = float(np.abs(np.asarray(cloud, np.float64)).max())
    return tuple(float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()) / scale for a, b in zip(got, ref))


# ---- whole encoders -----------------------------------------------------------------------------------------------------------------
LATENT_2D = [(1, 1), (2, 1), (1, 7), (5, 13), (3, 43), (3, 50), (1, 64), (1, 65), (6, 64), (16, 64)]
# (21, 200): 4200 points x 256 channels = 1,075,200 elements, past the 4096 x 256 elements one sweep of the grid-stride kernels covers
LATENT_3D = [(1, 1), (2, 1), (1, 5), (5, 50), (64, 3), (65, 2), (130, 1), (20, 200), (21, 200)]
SHARP_GAIN = 6.0


def latent_cloud(o3, no, npts):
    return synth.make_cloud(no, npts, 3 if o3 else 2, seed=1000 + 500 * int(o3) + 37 * no + npts)


def _coords_x4():
    return latent_cloud(False, 5, 13) * np.float32(4.0)


def _tiny_obstacle(order=None):
    """Obstacle 0 shrunk to 1e-3 of its size (2.6e-4 across) around its first point, after the point nearest the origin (|x| < 0.04) was
    put first.  Why there: float32 rounds the centre by about an ulp of the coordinates, and the normalisation divides by the obstacle's
    size; at |x| ~ 0.5 that alone moves the float32 oracle 1e-5 away from float64 and the figure changes with the order of the sum, near
    the origin it stays near 1e-6 in any order (`order` permutes the obstacle's points: test_scene_ref_host.py)."""
    c = latent_cloud(False, 3, 43).copy()
    o = c[0].copy()
    i = int(np.abs(o).max(-1).argmin())
    o[[0, i]] = o[[i, 0]]
    o = o[:1] + (o - o[:1]) * np.float32(1e-3)
    c[0] = o if order is None else o[order]
    return c


def identical_inexact_cloud():
    """An obstacle of 16 identical points at coordinates float32 cannot represent, beside an ordinary one.  NOT an accuracy case: the
    float32 mean is an ulp off the point, the normalisation divides that by 1e-8, and the float32 oracle itself is 2.3e-2 away from
    float64.  The GPU test asserts a finite latent only."""
    c = latent_cloud(False, 2, 16).copy()
    c[1] = np.asarray(IDENTICAL_INEXACT_POINT, np.float32)
    return c


# name -> (3-D?, sharp weights?, cloud factory)
LATENT_CASES = OrderedDict()
for _no, _np in LATENT_2D:
    LATENT_CASES[f"2d_{_no}x{_np}"] = (False, False, lambda no=_no, n=_np: latent_cloud(False, no, n))
for _no, _np in LATENT_3D:
    LATENT_CASES[f"3d_{_no}x{_np}"] = (True, False, lambda no=_no, n=_np: latent_cloud(True, no, n))
LATENT_CASES["2d_sharp_3x43"] = (False, True, lambda: latent_cloud(False, 3, 43))
LATENT_CASES["3d_sharp_70x3"] = (True, True, lambda: latent_cloud(True, 70, 3))
LATENT_CASES["2d_coords_x4"] = (False, False, _coords_x4)
LATENT_CASES["2d_tiny_obstacle"] = (False, False, _tiny_obstacle)

_SD, _ORACLE, _LAT = {}, {}, {}


def state_dict(o3, sharp=False):
    """The suite's synthetic weights; sharp: every scene-encoder attention input projection (2-D *.attn.qkv.weight, 3-D
    *.mha.in_proj_weight) times SHARP_GAIN."""
    key = (o3, sharp)
    if key not in _SD:
        sd = weights(6 if o3 else 4, 48, o3)
        if sharp:
            tail = ".mha.in_proj_weight" if o3 else ".attn.qkv.weight"
            sd = OrderedDict((k, v * np.float32(SHARP_GAIN) if k.startswith("scene_encoder.") and k.endswith(tail) else v) for k, v in sd.items())
            assert sum(k.endswith(tail) for k in sd) == (2 if o3 else 9)
        _SD[key] = sd
    return _SD[key]


def oracle(o3, sharp, dtype):
    from oracle import ramp_oracle as O
    key = (o3, sharp, np.dtype(dtype).name)
    if key not in _ORACLE:
        _ORACLE[key] = O.UNetOracle(state_dict(o3, sharp), 6 if o3 else 4, 48, obstacle_3d=o3, dtype=dtype)
    return _ORACLE[key]


def latent_case(name):
    """cloud, the float64 oracle's latent, the float32 oracle's and its error; computed once per process and left unchanged."""
    if name not in _LAT:
        o3, sharp, make = LATENT_CASES[name]
        cloud = make()
        lat64 = oracle(o3, sharp, np.float64).encode_scene(cloud)
        lat32 = oracle(o3, sharp, np.float32).encode_scene(cloud)
        for a in (cloud, lat64, lat32):
            a.setflags(write=False)
        _LAT[name] = dict(name=name, o3=o3, sharp=sharp, cloud=cloud, lat=lat64, lat32=lat32, floor=rel(lat32, lat64))
    return _LAT[name]
