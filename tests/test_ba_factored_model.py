"""CPU-only: the algebra of the factored bundle-adjustment build / update (csrc/vo_ba_factored.hip) in numpy, against the direct camera
blocks of oracle/ba_oracle.py (jacobian_blocks: Jp = [-A R [X]x Jr | A], Jl = A R).

With j_k = [X x Jl_k ; Jl_k] and T_s = blockdiag(Jr_s, R_s^T) the camera block is Jp_k = j_k^T T_s, so everything the build sums over the
observations of a camera can be summed in the basis of j_k from the landmark block P = w sum_k Jl_k Jl_k^T and gamma = w sum_k Jl_k e_k alone,
and T applied once afterwards.  Every identity to 1e-12 relative (float64 products of well-scaled 3 x 3 and 6 x 6 blocks: ~1e-15)."""
import numpy as np
import pytest

import ba_oracle as bo

TOL = 1e-12


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def scene(W, N, seed):
    """cameras with rotations far from the identity (Jr far from I), landmarks in front of them, outliers beyond the Huber knee, slots not observed"""
    rng = np.random.default_rng(seed)
    K = np.array([[718.856, 0.0, 607.19], [0.0, 718.856, 185.22], [0.0, 0.0, 1.0]])
    X = np.stack([rng.uniform(-8, 8, N), rng.uniform(-3, 3, N), rng.uniform(12, 40, N)], 1)
    Q = bo.rodrigues_exp([0.7, -1.1, 0.4])                 # world frame turned against the cameras'
    poses = np.zeros((W, 6))
    for i in range(W):
        poses[i, :3] = rng.normal(0, 0.02, 3)
        poses[i, 3:] = [0.1 * i, 0.02 * i, -0.8 * i] + rng.normal(0, 0.05, 3)
    Xw = X @ Q.T                                            # X_cam = R (Q^T X_w) + t: pose rotation R Q^T
    for i in range(W):
        R = bo.rodrigues_exp(poses[i, :3]) @ Q.T
        th = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
        poses[i, :3] = th / (2 * np.sin(th)) * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    obs = np.zeros((W, N, 2))
    for i in range(W):
        obs[i] = bo.project(K, poses[i], Xw)[0] + rng.normal(0, 0.4, (N, 2))
    obs[rng.uniform(size=(W, N)) < 0.2] = np.nan            # unobserved
    obs[0, 0] = np.nan                                      # (at least one)
    obs[1, 1] += 25.0                                       # beyond the knee: w < 1
    Xw = Xw + rng.normal(0, 0.2, Xw.shape)
    return K, poses, Xw, obs


def blocks(K, poses, X, obs):
    e, Jp, Jl, m = bo.jacobian_blocks(K, poses, X, obs)
    w = bo.huber_weight((e * e).sum(-1)) * m
    W, N = m.shape
    P = np.einsum('wn,wnka,wnkb->wnab', w, Jl, Jl)          # the observation's landmark block
    gam = np.einsum('wn,wnka,wnk->wna', w, Jl, e)
    T = np.zeros((W, 6, 6))
    for s in range(W):
        T[s, :3, :3] = bo.right_jacobian(poses[s, :3])
        T[s, 3:, 3:] = bo.rodrigues_exp(poses[s, :3]).T
    return e, Jp, Jl, m, w, P, gam, T, bo.skew(X)


@pytest.mark.parametrize("W,N,seed", [(10, 7, 0), (9, 5, 1), (10, 13, 2)])
def test_camera_block_is_the_landmark_block_in_another_basis(W, N, seed):
    K, poses, X, obs = scene(W, N, seed)
    e, Jp, Jl, m, w, P, gam, T, SX = blocks(K, poses, X, obs)
    assert (~m).any() and (w[m] < 1).any()
    for s in range(W):
        for l in range(N):
            jh = np.concatenate([np.cross(X[l], Jl[s, l]), Jl[s, l]], axis=1)        # [2, 6]: rows j_k^T
            if not m[s, l]:
                assert not Jp[s, l].any() and not jh.any() and not P[s, l].any() and not gam[s, l].any()
                continue
            assert rel(jh @ T[s], Jp[s, l]) <= TOL


@pytest.mark.parametrize("W,N,seed", [(10, 7, 0), (9, 5, 1), (10, 13, 2)])
def test_camera_sums_rotate_back(W, N, seed):
    """T^T H^ T and T^T g^ against sum w Jp^T Jp and sum w Jp^T e"""
    K, poses, X, obs = scene(W, N, seed)
    e, Jp, Jl, m, w, P, gam, T, SX = blocks(K, poses, X, obs)
    ne = bo.normal_equations(K, poses, X, obs)
    for s in range(W):
        Hh, gh = np.zeros((6, 6)), np.zeros(6)
        for l in range(N):
            M = SX[l] @ P[s, l]
            Hh += np.block([[M @ SX[l].T, M], [M.T, P[s, l]]])
            gh += np.concatenate([np.cross(X[l], gam[s, l]), gam[s, l]])
        assert rel(T[s].T @ Hh @ T[s], ne["Hpp"][s]) <= TOL
        assert rel(T[s].T @ gh, ne["gp"][s]) <= TOL


@pytest.mark.parametrize("W,N,seed", [(10, 7, 0), (9, 5, 1), (10, 13, 2)])
def test_gram_matrix_of_the_panel_rotates_back(W, N, seed):
    """TT^T (sum Y^ Y^^T) TT against sum Y Y^T, Y = [H_pl Cinv^T | Cinv g_l] as the build kernels stage it (column 6 W = y untouched)"""
    K, poses, X, obs = scene(W, N, seed)
    e, Jp, Jl, m, w, P, gam, T, SX = blocks(K, poses, X, obs)
    ne = bo.normal_equations(K, poses, X, obs)
    lam, n = 1e-3, 6 * W
    G, Gh = np.zeros((n + 1, n + 1)), np.zeros((n + 1, n + 1))
    TT = np.zeros((n + 1, n + 1)); TT[n, n] = 1.0
    for s in range(W):
        TT[6 * s:6 * s + 6, 6 * s:6 * s + 6] = T[s]
    for l in range(N):
        Hd = ne["Hll"][l].copy()
        Hd[np.arange(3), np.arange(3)] += lam * np.maximum(np.diag(ne["Hll"][l]), 1e-12)
        Cinv = np.linalg.inv(np.linalg.cholesky(Hd))
        Y, Yh = np.zeros((3, n + 1)), np.zeros((3, n + 1))
        for s in range(W):
            Z = w[s, l] * Jl[s, l] @ Cinv.T                                         # [2, 3]
            Y[:, 6 * s:6 * s + 6] = (Jp[s, l].T @ Z).T
            Q = P[s, l] @ Cinv.T
            Yh[:, 6 * s:6 * s + 3] = (SX[l] @ Q).T
            Yh[:, 6 * s + 3:6 * s + 6] = Q.T
            assert rel(Q, (w[s, l] * Jl[s, l]).T @ Jl[s, l] @ Cinv.T) <= TOL if m[s, l] else not Q.any()
        Y[:, n] = Yh[:, n] = Cinv @ ne["gl"][l]
        G += Y.T @ Y
        Gh += Yh.T @ Yh
    assert rel(TT.T @ Gh @ TT, G) <= TOL
    assert np.array_equal((TT.T @ Gh @ TT)[n, n], Gh[n, n])
    # ... which is the Schur complement and right-hand side the solve assembles: S = Hpp + lam D - E, rhs = -gp + r
    S, rhs, _, _, _ = bo.schur_system(ne, lam)
    Gr = TT.T @ Gh @ TT
    E = Gr[:n, :n]
    Sd = np.zeros((n, n))
    for s in range(W):
        blk = ne["Hpp"][s].copy()
        blk[np.arange(6), np.arange(6)] += lam * np.maximum(np.diag(ne["Hpp"][s]), 1e-12)
        Sd[6 * s:6 * s + 6, 6 * s:6 * s + 6] = blk
    assert rel(Sd - E, S) <= 1e-10 and rel(-ne["gp"].reshape(-1) + Gr[:n, n], rhs) <= 1e-10     # (S cancels: the oracle's own rounding)


@pytest.mark.parametrize("W,N,seed", [(10, 7, 0), (9, 5, 1), (10, 13, 2)])
def test_update_forms_jp_dp_from_the_landmark_block(W, N, seed):
    """Jp_s d_s = Jl z and w Jl^T Jp_s d_s = P z with z = R_s^T d_trans + (Jr_s d_rot) x X"""
    K, poses, X, obs = scene(W, N, seed)
    e, Jp, Jl, m, w, P, gam, T, SX = blocks(K, poses, X, obs)
    d = np.random.default_rng(seed + 100).normal(0, 0.05, (W, 6))
    for s in range(W):
        a, b = T[s, 3:, 3:] @ d[s, 3:], T[s, :3, :3] @ d[s, :3]
        for l in range(N):
            z = a + np.cross(b, X[l])
            if not m[s, l]:
                assert not (P[s, l] @ z).any()
                continue
            assert rel(Jl[s, l] @ z, Jp[s, l] @ d[s]) <= TOL
            assert rel(P[s, l] @ z, w[s, l] * Jl[s, l].T @ (Jp[s, l] @ d[s])) <= TOL
