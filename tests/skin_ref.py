"""TEST INFRASTRUCTURE: a numpy float64 restatement of the rig arithmetic (include/take_hip.h), written
from the specification operation by operation: every + - * / below is one elementwise IEEE operation over all vertices
at once, in the order the specification writes them; no einsum, no @, no sum().  Also the case list the CPU and the
GPU tests share (cases()), made from a seed."""
import numpy as np


def palette(joint_xforms, inverse_bind):
    """J_j = X_j · B_j as 3x4 affine matrices; inverse_bind None: J_j = X_j"""
    X = np.asarray(joint_xforms, np.float64).reshape(-1, 3, 4)
    if inverse_bind is None:
        return X.copy()
    B = np.asarray(inverse_bind, np.float64).reshape(-1, 3, 4)
    J = np.zeros_like(X)
    for r in range(3):
        for c in range(4):
            s = (X[:, r, 0] * B[:, 0, c] + X[:, r, 1] * B[:, 1, c]) + X[:, r, 2] * B[:, 2, c]
            if c == 3:
                s = s + X[:, r, 3]
            J[:, r, c] = s
    return J


def pose(positions, normals=None, joints=None, weights=None, inverse_bind=None, target_positions=None, target_normals=None,
         joint_xforms=None, target_weights=None):
    """-> (posed positions, posed normals or None)"""
    p = [np.array(np.asarray(positions, np.float64)[:, a]) for a in range(3)]
    n = None if normals is None else [np.array(np.asarray(normals, np.float64)[:, a]) for a in range(3)]
    # 1. morph
    if target_positions is not None:
        tp = np.asarray(target_positions, np.float64)
        tn = None if target_normals is None else np.asarray(target_normals, np.float64)
        for t in range(tp.shape[0]):
            w = np.float64(target_weights[t])
            for a in range(3):
                p[a] = p[a] + w * tp[t, :, a]
            if n is not None and tn is not None:
                for a in range(3):
                    n[a] = n[a] + w * tn[t, :, a]
    if joints is not None:
        # 2. blend
        J = palette(joint_xforms, inverse_bind)
        joints, weights = np.asarray(joints), np.asarray(weights, np.float64)
        M = [[weights[:, 0] * J[joints[:, 0], r, c] for c in range(4)] for r in range(3)]
        for k in range(1, joints.shape[1]):
            for r in range(3):
                for c in range(4):
                    M[r][c] = M[r][c] + weights[:, k] * J[joints[:, k], r, c]
        # 3. position
        p = [((M[r][0] * p[0] + M[r][1] * p[1]) + M[r][2] * p[2]) + M[r][3] for r in range(3)]
        # 4. normal: the cofactor matrix, C[i][j] = A[i+1][j+1] A[i+2][j+2] - A[i+1][j+2] A[i+2][j+1], indices mod 3
        if n is not None:
            Cf = [[M[(i + 1) % 3][(j + 1) % 3] * M[(i + 2) % 3][(j + 2) % 3] - M[(i + 1) % 3][(j + 2) % 3] * M[(i + 2) % 3][(j + 1) % 3]
                   for j in range(3)] for i in range(3)]
            det = (M[0][0] * Cf[0][0] + M[0][1] * Cf[0][1]) + M[0][2] * Cf[0][2]
            q = [(Cf[r][0] * n[0] + Cf[r][1] * n[1]) + Cf[r][2] * n[2] for r in range(3)]
            n = [np.where(det < 0, -q[r], q[r]) for r in range(3)]
    out_n = None
    if n is not None:
        with np.errstate(all="ignore"):
            length = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
            ok = (length > 0) & np.isfinite(length)
            out_n = np.stack([np.where(ok, n[a] / np.where(ok, length, 1.0), n[a]) for a in range(3)], axis=1)
    return np.stack(p, axis=1), out_n


def affine(rng, scale=(1.0, 1.0, 1.0)):
    """a 3x4 matrix: a random rotation times diag(scale), a random translation"""
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return np.concatenate([q * np.asarray(scale, np.float64)[None, :], rng.uniform(-1, 1, (3, 1))], axis=1)


def make_case(nv, nj, K, T, normals=True, target_normals=True, bind=True, seed=0, kind="plain"):
    """the arguments of pose() for one case.  kind: "plain"; "mirror" (joint 0 mirrored: det < 0); "scale" (joints scaled
    non-uniformly); "zero_normal" (some rest normals (0, 0, 0)); "unnormalised" (weights that do not sum to 1)"""
    rng = np.random.default_rng([seed, nv, nj, K, T])
    c = {"positions": rng.uniform(-1, 1, (nv, 3))}
    if normals:
        nrm = rng.standard_normal((nv, 3))
        c["normals"] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
        if kind == "zero_normal":
            c["normals"][::3] = 0.0
    if nj > 0:
        used = int(rng.integers(1, K + 1)) if K > 1 else 1  # the other influences are padding: weight 0 on a valid joint
        c["joints"] = rng.integers(0, nj, (nv, K)).astype(np.int32)
        w = rng.uniform(0.1, 1.0, (nv, K))
        w[:, used:] = 0.0
        w = w / w.sum(axis=1, keepdims=True)
        if kind == "unnormalised":
            w = w * rng.uniform(0.5, 1.5, (nv, 1))
        c["weights"] = w
        scales = [(1.0, 1.0, 1.0)] * nj
        if kind == "scale":
            scales = [tuple(rng.uniform(0.3, 3.0, 3)) for _ in range(nj)]
        if kind == "mirror":
            scales[0] = (-1.0, 1.0, 1.0)
            c["joints"][:, 0] = np.where(np.arange(nv) % 2 == 0, 0, c["joints"][:, 0])
        c["joint_xforms"] = np.stack([affine(rng, s) for s in scales])
        if bind:
            c["inverse_bind"] = np.stack([affine(rng) for _ in range(nj)])
    if T > 0:
        c["target_positions"] = rng.uniform(-0.1, 0.1, (T, nv, 3))
        if normals and target_normals:
            c["target_normals"] = rng.uniform(-0.1, 0.1, (T, nv, 3))
        c["target_weights"] = rng.uniform(-0.5, 1.0, T)
    return c


SIZES = (1, 63, 64, 65, 257, 1301)


def cases(lds_max_joints=None):
    """[(name, grid, case)]: grid 0 = the launch's own.  Every size with a few rigs; the 1301 with every K, T, joint
    count (both sides of the kernel's LDS threshold when it has one) and grids of 1-3 blocks; the inputs chosen to
    break things."""
    out = []
    for nv in SIZES:
        out.append((f"nv{nv}-k4-t1", 0, make_case(nv, 5, 4, 1)))
        out.append((f"nv{nv}-morph-only", 0, make_case(nv, 0, 0, 3)))
        out.append((f"nv{nv}-k1-no-normals", 0, make_case(nv, 2, 1, 0, normals=False, bind=False)))
    joint_counts = [1, 2] + ([lds_max_joints, lds_max_joints + 1] if lds_max_joints else [])
    nv = 1301
    for grid in (1, 2, 3):
        out.append((f"grid{grid}", grid, make_case(nv, 7, 4, 3, seed=grid)))
    for K in (1, 4, 8):
        for T in (0, 1, 3):
            for tn in (True, False):
                if T == 0 and not tn:
                    continue
                out.append((f"k{K}-t{T}-tn{int(tn)}", 0, make_case(nv, 9, K, T, target_normals=tn, bind=(K != 4))))
    for nj in joint_counts:
        out.append((f"nj{nj}", 0, make_case(257, nj, 4, 1)))
        out.append((f"nj{nj}-no-bind", 2, make_case(1301, nj, 8, 0, bind=False)))
    for kind in ("mirror", "scale", "zero_normal", "unnormalised"):
        out.append((kind, 0, make_case(257, 6, 4, 0 if kind == "zero_normal" else 1, kind=kind)))  # (no target moves a zero normal)
    return out
