"""Pose graphs and their optimisation, mirroring the Open3D calls of the reference
(make_fragments.py:254-265, refine_fragment_poses.py:297-308):

    o3d.pipelines.registration.PoseGraph / PoseGraphNode / PoseGraphEdge
    o3d.pipelines.registration.GlobalOptimizationOption(max_correspondence_distance, edge_prune_threshold,
                                                        preference_loop_closure, reference_node)
    o3d.pipelines.registration.GlobalOptimizationConvergenceCriteria()
    o3d.pipelines.registration.global_optimization(pose_graph, method, criteria, option)

The graphs have at most a few hundred nodes: this is host work in numpy float64, vectorised over the
edges (no Python loop over edges inside an iteration).  The rules -- pose vector, edge misalignment,
line process, linearisation, Levenberg-Marquardt schedule, the two passes with pruning between them --
are written out in DESIGN "pose-graph rules"; they restate Open3D's optimiser from memory and are not
pinned against it.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np


# ---- containers (Open3D's attribute names) ------------------------------------------------------------
# to_legacy() gives the real o3d.pipelines.registration objects when open3d imports (as mqr.geometry does).
@dataclass
class PoseGraphNode:
    pose: np.ndarray = field(default_factory=lambda: np.eye(4))

    def to_legacy(self):
        from .geometry import _try_open3d
        o3d = _try_open3d()
        return self if o3d is None else o3d.pipelines.registration.PoseGraphNode(pose=np.asarray(self.pose))


@dataclass
class PoseGraphEdge:
    source_node_id: int = -1
    target_node_id: int = -1
    transformation: np.ndarray = field(default_factory=lambda: np.eye(4))
    information: np.ndarray = field(default_factory=lambda: np.eye(6))
    uncertain: bool = False
    confidence: float = 1.0

    def to_legacy(self):
        from .geometry import _try_open3d
        o3d = _try_open3d()
        if o3d is None:
            return self
        return o3d.pipelines.registration.PoseGraphEdge(
            source_node_id=self.source_node_id, target_node_id=self.target_node_id,
            transformation=np.asarray(self.transformation), information=np.asarray(self.information),
            uncertain=self.uncertain, confidence=self.confidence)


@dataclass
class PoseGraph:
    nodes: List[PoseGraphNode] = field(default_factory=list)
    edges: List[PoseGraphEdge] = field(default_factory=list)

    def to_legacy(self):
        from .geometry import _try_open3d
        o3d = _try_open3d()
        if o3d is None:
            return self
        g = o3d.pipelines.registration.PoseGraph()
        for n in self.nodes:
            g.nodes.append(n.to_legacy())
        for e in self.edges:
            g.edges.append(e.to_legacy())
        return g


@dataclass
class GlobalOptimizationOption:
    max_correspondence_distance: float = 0.075
    edge_prune_threshold: float = 0.25
    preference_loop_closure: float = 1.0
    reference_node: int = -1


@dataclass
class GlobalOptimizationConvergenceCriteria:
    max_iteration: int = 100
    min_relative_increment: float = 1e-6
    min_relative_residual_increment: float = 1e-6
    min_right_term: float = 1e-6
    min_residual: float = 1e-6
    max_iteration_lm: int = 20
    upper_scale_factor: float = 2.0 / 3.0  # held for call compatibility; the stated schedule reads lower_scale_factor only
    lower_scale_factor: float = 1.0 / 3.0


class GlobalOptimizationLevenbergMarquardt:
    """The one method (accepted by global_optimization for call compatibility)."""


# ---- pose vector ----------------------------------------------------------------------------------------
def vec6(T) -> np.ndarray:
    """(..., 4, 4) -> (..., 6): (rx, ry, rz, tx, ty, tz) with R = Rz(rz) Ry(ry) Rx(rx)."""
    T = np.asarray(T, np.float64)
    R = T[..., :3, :3]
    sy = np.sqrt(R[..., 0, 0] ** 2 + R[..., 1, 0] ** 2)
    reg = sy > 1e-6
    rx = np.where(reg, np.arctan2(R[..., 2, 1], R[..., 2, 2]), np.arctan2(-R[..., 1, 2], R[..., 1, 1]))
    ry = np.arctan2(-R[..., 2, 0], sy)
    rz = np.where(reg, np.arctan2(R[..., 1, 0], R[..., 0, 0]), 0.0)
    return np.stack([rx, ry, rz, T[..., 0, 3], T[..., 1, 3], T[..., 2, 3]], -1)


def mat4(v) -> np.ndarray:
    """(..., 6) -> (..., 4, 4): the inverse of vec6."""
    v = np.asarray(v, np.float64)
    cx, sx = np.cos(v[..., 0]), np.sin(v[..., 0])
    cy, sy = np.cos(v[..., 1]), np.sin(v[..., 1])
    cz, sz = np.cos(v[..., 2]), np.sin(v[..., 2])
    T = np.zeros(v.shape[:-1] + (4, 4))
    T[..., 0, 0], T[..., 0, 1], T[..., 0, 2] = cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx
    T[..., 1, 0], T[..., 1, 1], T[..., 1, 2] = sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx
    T[..., 2, 0], T[..., 2, 1], T[..., 2, 2] = -sy, cy * sx, cy * cx
    T[..., 0, 3], T[..., 1, 3], T[..., 2, 3] = v[..., 3], v[..., 4], v[..., 5]
    T[..., 3, 3] = 1.0
    return T


def _rigid_inverse(T):
    R, t = T[..., :3, :3], T[..., :3, 3]
    out = np.zeros_like(T)
    Rt = np.swapaxes(R, -1, -2)
    out[..., :3, :3] = Rt
    out[..., :3, 3] = -(Rt @ t[..., None])[..., 0]
    out[..., 3, 3] = 1.0
    return out


def _generators():
    G = np.zeros((6, 4, 4))
    G[0, 1, 2], G[0, 2, 1] = -1.0, 1.0
    G[1, 0, 2], G[1, 2, 0] = 1.0, -1.0
    G[2, 0, 1], G[2, 1, 0] = -1.0, 1.0
    G[3, 0, 3] = G[4, 1, 3] = G[5, 2, 3] = 1.0
    return G


_G = _generators()


def _lin(M):
    return np.stack([(M[..., 2, 1] - M[..., 1, 2]) / 2, (M[..., 0, 2] - M[..., 2, 0]) / 2,
                     (M[..., 1, 0] - M[..., 0, 1]) / 2, M[..., 0, 3], M[..., 1, 3], M[..., 2, 3]], -1)


# ---- one Levenberg-Marquardt pass -------------------------------------------------------------------------
class _Problem:
    """The edges of one pass as arrays: s, t (E,), Xinv (E, 4, 4), L (E, 6, 6), uncertain (E,) bool."""

    def __init__(self, edges, n_nodes, option, ref):
        self.n = n_nodes
        self.ref = ref
        self.s = np.array([e.source_node_id for e in edges], np.int64)
        self.t = np.array([e.target_node_id for e in edges], np.int64)
        if len(edges) and (min(self.s.min(), self.t.min()) < 0 or max(self.s.max(), self.t.max()) >= n_nodes):
            raise ValueError("a pose-graph edge names a node that does not exist")
        X = np.stack([np.asarray(e.transformation, np.float64) for e in edges]) if edges else np.zeros((0, 4, 4))
        self.Xinv = _rigid_inverse(X)
        self.L = np.stack([np.asarray(e.information, np.float64) for e in edges]) if edges else np.zeros((0, 6, 6))
        self.unc = np.array([bool(e.uncertain) for e in edges], bool)
        self.mu = (option.preference_loop_closure * option.max_correspondence_distance ** 2
                   * float(self.L[:, 5, 5].mean())) if len(edges) else 0.0

    def errors(self, poses):
        """(A = X^-1 T_t^-1, e (E, 6), e^T L e (E,))"""
        A = self.Xinv @ _rigid_inverse(poses[self.t])
        e = vec6(A @ poses[self.s])
        return A, e, np.einsum("ei,eij,ej->e", e, self.L, e)

    def line_process(self, q):
        l = np.ones(len(q))
        if self.unc.any():
            l[self.unc] = (self.mu / (self.mu + q[self.unc])) ** 2
        return l

    def residual(self, q, l):
        return float((l * q).sum() + self.mu * ((np.sqrt(l[self.unc]) - 1.0) ** 2).sum())

    def linearise(self, poses, A, e, l):
        """(H (6n, 6n), b (6n,)) with the reference node's rows and columns replaced by the identity."""
        n = self.n
        GT = _G[None] @ poses[self.s][:, None]                      # (E, 6, 4, 4): G_k T_s
        Js = np.swapaxes(_lin(A[:, None] @ GT), 1, 2)               # (E, 6, 6): column k = lin(A G_k T_s)
        LJ = l[:, None, None] * (self.L @ Js)                       # l L J_s
        JLJ = np.swapaxes(Js, 1, 2) @ LJ                            # l J_s^T L J_s; J_t = -J_s
        Hb = np.zeros((n, n, 6, 6))
        np.add.at(Hb, (self.s, self.s), JLJ)
        np.add.at(Hb, (self.t, self.t), JLJ)
        np.add.at(Hb, (self.s, self.t), -JLJ)
        np.add.at(Hb, (self.t, self.s), -JLJ)
        g = np.einsum("eji,ej->ei", LJ, e)                          # l J_s^T L e
        bb = np.zeros((n, 6))
        np.add.at(bb, self.s, -g)
        np.add.at(bb, self.t, g)
        H = Hb.transpose(0, 2, 1, 3).reshape(6 * n, 6 * n)
        b = bb.reshape(6 * n)
        r = slice(6 * self.ref, 6 * self.ref + 6)
        H[r, :] = 0.0
        H[:, r] = 0.0
        H[r, r] = np.eye(6)
        b[r] = 0.0
        return H, b


def _optimise(poses, prob, criteria):
    """One pass from l = 1.  Returns (poses, l, report)."""
    E = len(prob.s)
    report = {"residuals": [], "iterations": 0, "edges": E}
    l = np.ones(E)
    if E == 0:
        return poses, l, report
    A, e, q = prob.errors(poses)
    r = prob.residual(q, l)
    report["residuals"].append(r)
    H, b = prob.linearise(poses, A, e, l)
    lam = 1e-5 * float(np.diag(H).max())
    nu = 2.0
    n6 = 6 * prob.n
    ref = prob.ref
    stop = float(np.abs(b).max()) <= criteria.min_right_term
    for _ in range(criteria.max_iteration):
        if stop:
            break
        report["iterations"] += 1
        tries = 0
        while True:
            delta = np.linalg.solve(H + lam * np.eye(n6), b)
            x = vec6(poses).reshape(-1)
            if np.linalg.norm(delta) <= criteria.min_relative_increment * (np.linalg.norm(x) + criteria.min_relative_increment):
                stop = True
                break
            new = mat4(delta.reshape(-1, 6)) @ poses
            new[ref] = poses[ref]
            A2, e2, q2 = prob.errors(new)
            l2 = prob.line_process(q2)
            r2 = prob.residual(q2, l2)
            rho = (r - r2) / (float(delta @ (lam * delta + b)) + 1e-3)
            if rho > 0:
                if r - r2 < criteria.min_relative_residual_increment * r:
                    stop = True
                poses, l, r = new, l2, r2
                report["residuals"].append(r)
                H, b = prob.linearise(poses, A2, e2, l)
                stop = stop or float(np.abs(b).max()) <= criteria.min_right_term
                lam *= max(criteria.lower_scale_factor, 1.0 - (2.0 * rho - 1.0) ** 3)
                nu = 2.0
                break
            lam *= nu
            nu *= 2.0
            tries += 1
            if tries >= criteria.max_iteration_lm:
                break
        stop = stop or r < criteria.min_residual
    return poses, l, report


def global_optimization(pose_graph: PoseGraph, *args, option: Optional[GlobalOptimizationOption] = None,
                        criteria: Optional[GlobalOptimizationConvergenceCriteria] = None):
    """Optimise `pose_graph` in place: ``global_optimization(pose_graph, option, criteria=None)``, or
    Open3D's argument order ``(pose_graph, method, criteria, option)``.  Afterwards the nodes hold the
    optimised poses, ``pose_graph.edges`` the surviving edges, and each uncertain edge's ``confidence``
    its final line-process value.  Returns the two passes' reports (residual after every accepted step,
    iterations, edges)."""
    for a in args:
        if isinstance(a, GlobalOptimizationOption):
            option = a
        elif isinstance(a, GlobalOptimizationConvergenceCriteria):
            criteria = a
        elif a is not None and not isinstance(a, GlobalOptimizationLevenbergMarquardt):
            raise TypeError(f"unexpected argument of type {type(a).__name__}")
    if option is None:
        raise TypeError("global_optimization needs a GlobalOptimizationOption")
    criteria = criteria or GlobalOptimizationConvergenceCriteria()
    n = len(pose_graph.nodes)
    if n == 0:
        return []
    ref = 0 if option.reference_node < 0 else int(option.reference_node)
    if ref >= n:
        raise ValueError(f"reference_node {ref} is not a node of the graph")
    poses = np.stack([np.array(nd.pose, np.float64) for nd in pose_graph.nodes])
    edges = list(pose_graph.edges)
    poses, l, rep1 = _optimise(poses, _Problem(edges, n, option, ref), criteria)
    kept = [e for e, le in zip(edges, l) if not e.uncertain or le >= option.edge_prune_threshold]
    rep1["pruned"] = len(edges) - len(kept)
    for e, le in zip(edges, l):  # a pruned edge keeps the value it was pruned for
        if e.uncertain:
            e.confidence = float(le)
    poses, l, rep2 = _optimise(poses, _Problem(kept, n, option, ref), criteria)
    for e, le in zip(kept, l):
        if e.uncertain:
            e.confidence = float(le)
    for nd, T in zip(pose_graph.nodes, poses):
        nd.pose = T
    pose_graph.edges[:] = kept
    return [rep1, rep2]
