"""An independent forward dynamics of the robot's articulated chain in numpy float64, written
from the Lagrangian and sharing no code with the oracle or the kernels (no Newton-Euler recursion):

  * forward kinematics from the compiled scene's link arrays (rl_parent, rl_jtype, rl_dof,
    rl_jpos, rl_jquat, rl_axis, rl_com_pos, rl_com_quat), the base pose an argument;
  * M(q) = sum over links of m Jv^T Jv + Jw^T (R diag(I) R^T) Jw, the Jacobian columns of a link
    being those of its ancestor joints (revolute: Jw = axis, Jv = axis x (c - o); prismatic:
    Jv = axis);
  * the velocity-product forces from the Christoffel symbols of central differences of M
    (step 1e-5): c_k = sum_ij (dM_kj/dq_i - 1/2 dM_ij/dq_k) qd_i qd_j;
  * qdd = -M^-1 c: no gravity on the robot (the tasks zero it), no damping, no motors.

Everything is per state and unvectorised on purpose: it is read more often than it is run.
"""
import numpy as np

J_REVOLUTE, J_PRISMATIC = 1, 2        # the compiled scene's rl_jtype values (0: fixed)
DIFF_STEP = 1e-5


def quat_to_rot(q):
    """Rotation matrix of the unit quaternion (x, y, z, w)."""
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def axis_rot(axis, angle):
    """Rodrigues: the rotation by `angle` about the unit vector `axis`."""
    a = np.asarray(axis, np.float64)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def n_dof(A):
    return int(np.sum(np.asarray(A['rl_dof'])[:int(A['n_links'])] >= 0))


def kinematics(A, q, base):
    """Per link: the joint's world origin and axis, the COM's world position and the rotation of
    the principal inertia frame.  base: (x, y, z, qx, qy, qz, qw) of the fixed root."""
    nl = int(A['n_links'])
    base = np.asarray(base, np.float64)
    Rb, pb = quat_to_rot(base[3:7]), base[:3]
    Rl, pl = [None] * nl, [None] * nl
    org, axw, com, Rc = np.zeros((nl, 3)), np.zeros((nl, 3)), np.zeros((nl, 3)), np.zeros((nl, 3, 3))
    for i in range(nl):
        p = int(A['rl_parent'][i])
        assert p < i, 'links are listed parents first'
        Rp, pp = (Rb, pb) if p < 0 else (Rl[p], pl[p])
        R = Rp @ quat_to_rot(A['rl_jquat'][i])
        o = pp + Rp @ np.asarray(A['rl_jpos'][i], np.float64)
        a = np.asarray(A['rl_axis'][i], np.float64)
        org[i], axw[i] = o, R @ a
        t, d = int(A['rl_jtype'][i]), int(A['rl_dof'][i])
        if t == J_REVOLUTE:
            R = R @ axis_rot(a, q[d])
        elif t == J_PRISMATIC:
            o = o + axw[i] * q[d]
        Rl[i], pl[i] = R, o
        com[i] = o + R @ np.asarray(A['rl_com_pos'][i], np.float64)
        Rc[i] = R @ quat_to_rot(A['rl_com_quat'][i])
    return org, axw, com, Rc


def mass_matrix(A, q, base):
    nl, nd = int(A['n_links']), n_dof(A)
    org, axw, com, Rc = kinematics(A, q, base)
    M = np.zeros((nd, nd))
    for i in range(nl):
        m = float(A['rl_mass'][i])
        if m <= 0:
            continue
        Jv, Jw = np.zeros((3, nd)), np.zeros((3, nd))
        k = i
        while k >= 0:                                  # the link's own joint and its ancestors'
            t, d = int(A['rl_jtype'][k]), int(A['rl_dof'][k])
            if t == J_REVOLUTE:
                Jw[:, d] = axw[k]
                Jv[:, d] = np.cross(axw[k], com[i] - org[k])
            elif t == J_PRISMATIC:
                Jv[:, d] = axw[k]
            k = int(A['rl_parent'][k])
        Iw = Rc[i] @ np.diag(np.asarray(A['rl_inertia'][i], np.float64)) @ Rc[i].T
        M += m * Jv.T @ Jv + Jw.T @ Iw @ Jw
    return M


def mass_matrix_derivatives(A, q, base, h=DIFF_STEP):
    """dM[i] = dM/dq_i by central differences."""
    q = np.asarray(q, np.float64)
    nd = n_dof(A)
    dM = np.zeros((nd, nd, nd))
    for i in range(nd):
        e = np.zeros(nd)
        e[i] = h
        dM[i] = (mass_matrix(A, q + e, base) - mass_matrix(A, q - e, base)) / (2 * h)
    return dM


def bias(A, q, qd, base, h=DIFF_STEP):
    """c_k = sum_ij (dM_kj/dq_i - 1/2 dM_ij/dq_k) qd_i qd_j."""
    qd = np.asarray(qd, np.float64)
    dM = mass_matrix_derivatives(A, q, base, h)
    return np.einsum('ikj,i,j->k', dM, qd, qd) - 0.5 * np.einsum('kij,i,j->k', dM, qd, qd)


def forward_dynamics(A, q, qd, base):
    """(qdd, M, c) of the unforced, undamped chain."""
    M = mass_matrix(A, np.asarray(q, np.float64), base)
    c = bias(A, q, qd, base)
    return -np.linalg.solve(M, c), M, c
