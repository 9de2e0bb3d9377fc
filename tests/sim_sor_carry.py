"""Lane-level model of the ISSUE ORDER of the exact-order SOR steps since the operand slots carry the left weight and
the next centre (papteam_opticalflow_amd/csrc/sor.hip: step(), f_step(), refill(), unknowns_end()).  Layout, lanes and
arithmetic are those of tests/sim_sor_wave.py, whose helpers this module imports; what is modelled anew:

* slot t = s mod R of a task holds (phi, xy), (a1, a2, b1, b2) and (du, dv) right-old of step s.  Step s reads its left
  weight and its centre OUT OF THE SLOT OF STEP s - 1 (nothing is copied out of a slot), and at its end refills
  (a, b)[t] for step s + R but (phi, xy)[t - 1] and (du, dv)[t - 1] for step s + R - 1: the loads read memory at that
  moment, R - 1 steps before their use.  Slot R - 1 is carried from the last step of an iteration into step 0 of the
  next.  The fused pair kernel refills (du, dv)[t - 1] likewise, (a, b)[t - 2] for step s - 2 + R once s >= 2 and
  (phi, xy)[t - 3] for step s - 3 + R once s >= 3 (the second sweep's left weight is the phi of step s - 3);
* the coverage bound: the start-up requests the unknowns of steps < R - 1, iteration i those of steps
  < (i + 2) R - 1 =: e, and needs prog[k-1][b] >= min(NS, e + OWN), prog[k][b-1] >= min(NS, e + UP),
  prog[k-2][b+1] >= min(NS, e - 62) (OWN, UP = 0, 63; fused pairs 1, 64) -- `weaken` lowers e, to show that the bound
  is exact: with weaken = 1 a task reads a cell before it is written;
* the WEAKEST memory the protocol allows: a task's stores become visible only when a publication covers them (until
  then the plane holds NaN, or the value of two sweeps ago), a publication advertises any number of completed steps
  up to the real one (the kernel's markers prove particular values; a bound that holds for every value holds for
  those), and tasks advance ONE STEP at a time under a random scheduler.
"""
import numpy as np

from sim_sor_wave import FROWS, LANES, ROWS, layout, layout_fused, shift_down, shift_up, to_skew


def _update(st, phiL, duC, dvC, phiC, xy, a1, a2, b1, b2, duR, dvR, om1, nalpha):
    """the cell update of a lane-vector: left / up as products of the left weight (wave_cell() in sor.hip)"""
    duU, dvU, phiU = shift_up(st["duL"]), shift_up(st["dvL"]), shift_up(phiL)
    duD, dvD = shift_down(duR), shift_down(dvR)
    s1 = phiL * st["duL"]
    s2 = phiL * st["dvL"]
    s1 = s1 + phiC * duR
    s2 = s2 + phiC * dvR
    s1 = s1 + phiU * duU
    s2 = s2 + phiU * dvU
    s1 = s1 + phiC * duD
    s2 = s2 + phiC * dvD
    s1 = s1 * nalpha
    s2 = s2 * nalpha
    s1 = s1 + xy * dvC
    duN = om1 * duC + a1 * (b1 - s1)
    s2 = s2 + xy * duN
    dvN = om1 * dvC + a2 * (b2 - s2)
    return duN, dvN


class _Engine(object):
    """tasks, deferred stores, lagging publications and the one-step random scheduler shared by both kernels"""

    def __init__(self, nb, units, ns, r, npos_d, own, up, weaken, seed):
        self.nb, self.units, self.ns, self.r, self.own, self.up, self.weaken = nb, units, ns, r, own, up, weaken
        self.D = np.zeros((2, 2, npos_d, nb, LANES))  # [du|dv][parity][position][band][cell]
        self.D[:, :, :ns] = np.nan                     # only the tail positions are cleared between solves
        self.prog = np.zeros((nb, units), dtype=np.int64)
        self.rng = np.random.default_rng(seed)
        self.n_iter = (ns + r - 1) // r

    def unknowns_end(self, i):
        return (i + 2) * self.r - 1 - self.weaken

    def covered(self, b, u, e):
        ns, ok = self.ns, True
        if u > 0:
            ok = ok and self.prog[b, u - 1] >= min(ns, e + self.own)
        if b > 0:
            ok = ok and self.prog[b - 1, u] >= min(ns, e + self.up)
        if u > 1 and b + 1 < self.nb:
            ok = ok and self.prog[b + 1, u - 2] >= min(ns, max(0, e - 62))
        return ok

    def publish(self, t, steps):
        """advertise `steps` completed steps: their stores are visible from now on"""
        while t.pending and t.pending[0][0] < steps:
            _, pos, lanes, u_, v_ = t.pending.pop(0)
            self.D[0, t.u & 1, pos, t.b, lanes] = u_[lanes]
            self.D[1, t.u & 1, pos, t.b, lanes] = v_[lanes]
        self.prog[t.b, t.u] = steps

    def run(self, tasks, start, step):
        pending = list(tasks)
        while pending:
            ran = False
            for ti in self.rng.permutation(len(pending)):
                t = pending[ti]
                if t.s < 0:  # staged start-up
                    if not self.covered(t.b, t.u, self.unknowns_end(-1)):
                        continue
                    start(t)
                    t.s = 0
                    ran = True
                    break
                if t.s % self.r == 0 and not self.covered(t.b, t.u, self.unknowns_end(t.s // self.r)):
                    continue
                ran = True
                step(t, t.s)
                t.s += 1
                if t.s == self.n_iter * self.r:
                    self.publish(t, self.ns)  # after a full drain
                    assert not [p for p in t.pending if p[0] < self.ns]
                    pending.pop(ti)
                elif self.rng.random() < 0.3:  # a lagging publication: any value up to the steps really completed
                    self.publish(t, max(int(self.prog[t.b, t.u]), min(self.ns, int(self.rng.integers(0, t.s + 1)))))
                break
            assert ran, "deadlock in the task graph"


class _Task(object):
    def __init__(self, b, u, r):
        self.b, self.u, self.s = b, u, -1
        z = np.zeros(LANES)
        self.st = dict(duL=z.copy(), dvL=z.copy())
        self.st2 = dict(duL=z.copy(), dvL=z.copy(), duC=z.copy(), dvC=z.copy())
        self.c0 = None
        self.pa, self.ab, self.pd = [None] * r, [None] * r, [None] * r
        self.pending = []  # (step, position, lanes, du, dv) not yet visible


def simulate(phi, imdxy, a1, a2, b1, b2, n_sor, alpha, omega, r=8, seed=0, weaken=0):
    """`k_sor_exact<R>` in the new issue order.  Returns du, dv (H x W)."""
    h, w = phi.shape
    lay = layout(h, w, n_sor, r)
    nb, ns, rt, qt = lay["nb"], lay["ns"], lay["rt"], lay["qt"]
    P = {n: to_skew(p, lay) for n, p in dict(phi=phi, xy=imdxy, a1=a1, a2=a2, b1=b1, b2=b2).items()}
    npos_d = ns + 2 * r + 72
    E = _Engine(nb, n_sor, ns, r, npos_d, 0, 63, weaken, seed)
    D = E.D
    om1 = np.full(LANES, 1 - omega)
    om1[0] = om1[63] = 1.0
    real = np.zeros(LANES, dtype=bool)
    real[1:63] = True
    every = np.arange(LANES)

    def window(b, k):
        r0 = ROWS * b - k - 1
        return r0 + qt, slice(r0 + rt, r0 + rt + LANES)

    def load_pd(b, k, s):
        v = np.zeros((2, LANES))
        if k > 0 and s >= 0:
            v[:, 1:] = D[:, (k - 1) & 1, s + 1, b, :63]
        if b > 0 and s + 64 < npos_d:
            v[:, 0] = D[:, k & 1, s + 64, b - 1, 62]
        return v

    def load_phi(b, k, s):
        q0, rows = window(b, k)
        return P["phi"][q0 + s, rows].copy(), P["xy"][q0 + s, rows].copy()

    def load_ab(b, k, s):
        q0, rows = window(b, k)
        return tuple(np.where(real, P[n][q0 + s, rows], 0.0) for n in ("a1", "a2", "b1", "b2"))

    def start(t):
        t.c0 = load_pd(t.b, t.u, -1)
        for s in range(r):
            t.ab[s] = load_ab(t.b, t.u, s)
            if s < r - 1:
                t.pa[s] = load_phi(t.b, t.u, s)
                t.pd[s] = load_pd(t.b, t.u, s)

    def step(t, s):
        b, k, sl, tp = t.b, t.u, s % r, (s - 1) % r
        phiL = t.pa[tp][0] if s > 0 else np.zeros(LANES)  # out of the previous step's slot, not out of a copy
        cen = t.pd[tp] if s > 0 else t.c0
        phiC, xy = t.pa[sl]
        duN, dvN = _update(t.st, phiL, cen[0], cen[1], phiC, xy, *t.ab[sl], t.pd[sl][0], t.pd[sl][1], om1, -alpha)
        t.pending.append((s, s + 1, every, duN, dvN))
        t.st["duL"], t.st["dvL"] = duN, dvN
        t.pa[tp] = load_phi(b, k, s + r - 1)  # refill(): reads memory NOW
        t.ab[sl] = load_ab(b, k, s + r)
        t.pd[tp] = load_pd(b, k, s + r - 1)

    with np.errstate(invalid="ignore"):
        E.run([_Task(b, k, r) for k in range(n_sor) for b in range(nb)], start, step)
    kl = n_sor - 1
    ii, jj = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    bb, cc = (ii + kl) // ROWS, 1 + (ii + kl) % ROWS
    return D[0, kl & 1, jj + cc + 1, bb, cc], D[1, kl & 1, jj + cc + 1, bb, cc]


def simulate_fused(phi, imdxy, a1, a2, b1, b2, n_sor, alpha, omega, r=8, seed=0, weaken=0):
    """`k_sor_fused<R>` in the new issue order.  Returns du, dv (H x W)."""
    h, w = phi.shape
    lay = layout_fused(h, w, n_sor, r)
    nb, ns, rt, qt, last = lay["nb"], lay["ns"], lay["rt"], lay["qt"], lay["last"]
    pairs = last + 1
    P = {n: to_skew(p, lay) for n, p in dict(phi=phi, xy=imdxy, a1=a1, a2=a2, b1=b1, b2=b2).items()}
    npos_d = ns + 2 * r + 72
    E = _Engine(nb, pairs, ns, r, npos_d, 1, 64, weaken, seed)
    D = E.D
    lane = np.arange(LANES)
    real1 = (lane >= 2) & (lane <= 62)
    om1a = np.where(real1, 1 - omega, 1.0)
    om1b = np.where((lane == 0) | (lane == 63), 1.0, 1 - omega)
    coef_on = (lane != 0) & (lane != 63)
    stored = np.arange(LANES - 1)  # lane 63 does not store

    def window(b, q):
        r0 = FROWS * b - 2 * q - 2
        return r0 + qt, slice(r0 + rt, r0 + rt + LANES)

    def load_pd(b, q, s):
        v = np.zeros((2, LANES))
        if q > 0 and s >= 0:
            v[:, 2:] = D[:, (q - 1) & 1, s + 2, b, :62]
        if b > 0:
            if s + 63 < npos_d:
                v[:, 1] = D[:, q & 1, s + 63, b - 1, 62]
            if s + 65 < npos_d:
                v[:, 0] = D[:, q & 1, s + 65, b - 1, 61]
        return v

    def load_phi(b, q, s):
        q0, rows = window(b, q)
        return P["phi"][q0 + s, rows].copy(), P["xy"][q0 + s, rows].copy()

    def load_ab(b, q, s):
        q0, rows = window(b, q)
        return tuple(np.where(coef_on, P[n][q0 + s, rows], 0.0) for n in ("a1", "a2", "b1", "b2"))

    def start(t):
        t.c0 = load_pd(t.b, t.u, -1)
        for s in range(r):
            t.pa[s] = load_phi(t.b, t.u, s)
            t.ab[s] = load_ab(t.b, t.u, s)
            if s < r - 1:
                t.pd[s] = load_pd(t.b, t.u, s)

    def step(t, s):
        b, q = t.b, t.u
        sl, tp, t2, t3 = s % r, (s - 1) % r, (s - 2) % r, (s - 3) % r
        identity2 = (n_sor & 1) == 1 and q == pairs - 1
        duR2, dvR2 = t.st["duL"], t.st["dvL"]  # first-sweep results of step s - 1
        if s < 2:
            duN2, dvN2 = np.zeros(LANES), np.zeros(LANES)
        else:
            phiL2 = t.pa[t3][0] if s >= 3 else np.zeros(LANES)  # out of the slot of step s - 3
            a1_, a2_, b1_, b2_ = t.ab[t2]
            if identity2:  # (a1, a2) masked to zero, 1 - omega -> 1: the pass-through
                a1_, a2_, om2 = np.zeros(LANES), np.zeros(LANES), np.ones(LANES)
            else:
                om2 = om1b
            duN2, dvN2 = _update(t.st2, phiL2, t.st2["duC"], t.st2["dvC"], t.pa[t2][0], t.pa[t2][1], a1_, a2_, b1_, b2_,
                                 duR2, dvR2, om2, -alpha)
        phiL = t.pa[tp][0] if s > 0 else np.zeros(LANES)
        cen = t.pd[tp] if s > 0 else t.c0
        a1_, a2_, b1_, b2_ = t.ab[sl]
        a1m, a2m = np.where(real1, a1_, 0.0), np.where(real1, a2_, 0.0)
        duN, dvN = _update(t.st, phiL, cen[0], cen[1], t.pa[sl][0], t.pa[sl][1], a1m, a2m, b1_, b2_, t.pd[sl][0],
                           t.pd[sl][1], om1a, -alpha)
        t.pending.append((s, s + 1, stored, np.where(lane == 62, duN, duN2), np.where(lane == 62, dvN, dvN2)))
        t.st2["duL"], t.st2["dvL"], t.st2["duC"], t.st2["dvC"] = duN2, dvN2, duR2, dvR2
        t.st["duL"], t.st["dvL"] = duN, dvN
        t.pd[tp] = load_pd(b, q, s + r - 1)
        if s >= 3:
            t.pa[t3] = load_phi(b, q, s - 3 + r)
        if s >= 2:
            t.ab[t2] = load_ab(b, q, s - 2 + r)

    with np.errstate(invalid="ignore"):
        E.run([_Task(b, q, r) for q in range(pairs) for b in range(nb)], start, step)
    ii, jj = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    tt = ii + 2 * last + 1
    bb, cc = tt // FROWS, 1 + tt % FROWS
    return D[0, last & 1, jj + cc + 3, bb, cc], D[1, last & 1, jj + cc + 3, bb, cc]
