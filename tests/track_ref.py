"""Plot-to-track association from CPI to CPI, restated in plain numpy fp64 (include/rsp.h, "tracking";
DESIGN.md §4h): what rsp_track_dev must equal bit for bit.

  * Params / new_state / step / run: the seven steps of one CPI, with the association as the
    sequential greedy walk over the sorted keys.
  * associate_greedy / associate_rounds: the sequential form, and the rounds of mutual-best pairs
    the kernel runs (a second form, compared on every scene of CASES).
  * scene / quantised_scene: seeded scenes of moving targets and uniform false alarms, and of
    plots on a grid where equal costs are common.
  * CASES: the shapes the GPU test sweeps.  track_params / BAD_PARAMS: the C struct, and every
    parameter rsp_track_dev refuses.

Every floating-point operation is a separate numpy float64 operation in the order rsp.h writes it.
"""
import numpy as np

FREE, TENTATIVE, CONFIRMED = 0, 1, 2
# state_i columns
ID, STATUS, HIST, MISSES, HITS, AGE, LAST = range(7)
# tcount columns
LIVE, NCONF, STARTED, DROPPED, NOT_STARTED, N_VALID, MATCHED = range(7)


class Params:
    def __init__(self, max_tracks=64, confirm=(3, 5), drop=(2, 4), dt=0.08, rate_sign=1.0, gate=(30.0, 2.0),
                 alpha=(0.5, 0.5, 0.5)):
        self.max_tracks = int(max_tracks)
        self.M, self.N = int(confirm[0]), int(confirm[1])
        self.drop_t, self.drop_c = int(drop[0]), int(drop[1])
        self.dt, self.rate_sign = float(dt), float(rate_sign)
        self.gate_r, self.gate_v = float(gate[0]), float(gate[1])
        self.alpha_r, self.alpha_v, self.alpha_e = (float(x) for x in alpha)

    def kwargs(self):
        """The keyword arguments of rsp.track.Tracker that say the same."""
        return dict(max_tracks=self.max_tracks, confirm=(self.M, self.N), drop=(self.drop_t, self.drop_c), dt=self.dt,
                    rate_sign=self.rate_sign, gate=(self.gate_r, self.gate_v),
                    alpha=(self.alpha_r, self.alpha_v, self.alpha_e))


def new_state(slots, max_tracks):
    """(state_f [slots][T][4], state_i [slots][T][8], meta [slots][2]), all zero: every entry free."""
    return (np.zeros((slots, max_tracks, 4), np.float64), np.zeros((slots, max_tracks, 8), np.int32),
            np.zeros((slots, 2), np.int32))


def candidates(rp, vp, status, r, v, valid, p):
    """The in-gate pairs as (class, cost, t, j), unsorted."""
    wr = np.float64(1.0) / (np.float64(p.gate_r) * np.float64(p.gate_r))
    wv = np.float64(1.0) / (np.float64(p.gate_v) * np.float64(p.gate_v))
    out = []
    with np.errstate(invalid="ignore"):
        for t in np.flatnonzero(status != FREE):
            dr = r - rp[t]
            dv = v - vp[t]
            ok = valid & (np.abs(dr) <= p.gate_r) & (np.abs(dv) <= p.gate_v)
            c = ((dr * dr) * wr) + ((dv * dv) * wv)
            cls = 0 if status[t] == CONFIRMED else 1
            out.extend((cls, float(c[j]), int(t), int(j)) for j in np.flatnonzero(ok))
    return out


def associate_greedy(cands, T, n):
    """match [T] (plot or -1): the candidates in ascending key order, skipping taken tracks and plots."""
    match = np.full(T, -1, np.int64)
    taken = np.zeros(n, bool)
    for _, _, t, j in sorted(cands):
        if match[t] < 0 and not taken[j]:
            match[t] = j
            taken[j] = True
    return match


def associate_rounds(cands, T, n):
    """(match, rounds): every round matches each pair that is the smallest candidate of both its
    track and its plot among the still-free ones."""
    match = np.full(T, -1, np.int64)
    taken = np.zeros(n, bool)
    rounds = 0
    while True:
        free = [k for k in cands if match[k[2]] < 0 and not taken[k[3]]]
        if not free:
            return match, rounds
        best_t, best_j = {}, {}
        for k in free:
            if k[2] not in best_t or k < best_t[k[2]]:
                best_t[k[2]] = k
            if k[3] not in best_j or k < best_j[k[3]]:
                best_j[k[3]] = k
        for k in best_t.values():
            if best_j[k[3]] is k:
                match[k[2]] = k[3]
                taken[k[3]] = True
        rounds += 1


def step(sf, si, meta, est, n, p, h=None, associate=associate_greedy):
    """One CPI applied in place to one slot's state (sf [T][4], si [T][8], meta [2]); est [>= n][3].
    Returns (assign [n], tcount [8])."""
    T = p.max_tracks
    h = np.float64(p.dt if h is None else h)
    est = np.asarray(est, np.float64).reshape(-1, 3)[:n]
    r, v, ele = est[:, 0].copy(), est[:, 1].copy(), est[:, 2].copy()
    valid = ~(np.isnan(r) | np.isnan(v))
    status = si[:, STATUS].copy()
    live = status != FREE
    # 1 predict
    rp = sf[:, 0] + ((np.float64(p.rate_sign) * sf[:, 1]) * h)
    vp = sf[:, 1].copy()
    # 2, 3 gate and associate
    match = associate(candidates(rp, vp, status, r, v, valid, p), T, n)
    if isinstance(match, tuple):
        match = match[0]
    assign = np.where(valid, 0, -1).astype(np.int32)
    mask_n = 0xffffffff if p.N >= 32 else (1 << p.N) - 1
    dropped = matched = 0
    # 4, 5 update, confirm, drop
    for t in np.flatnonzero(live):
        j = int(match[t])
        hist = int(si[t, HIST]) & 0xffffffff
        if j >= 0:
            sf[t, 0] = rp[t] + np.float64(p.alpha_r) * (r[j] - rp[t])
            sf[t, 1] = vp[t] + np.float64(p.alpha_v) * (v[j] - vp[t])
            if np.isnan(ele[j]):
                pass
            elif np.isnan(sf[t, 2]):
                sf[t:t + 1, 2].view(np.int64)[:] = ele[j:j + 1].view(np.int64)
            else:
                sf[t, 2] = sf[t, 2] + np.float64(p.alpha_e) * (ele[j] - sf[t, 2])
            hist = ((hist << 1) | 1) & 0xffffffff
            si[t, MISSES] = 0
            si[t, HITS] += 1
            si[t, LAST] = j
            assign[j] = si[t, ID]
            matched += 1
        else:
            sf[t, 0] = rp[t]
            sf[t, 1] = vp[t]
            hist = (hist << 1) & 0xffffffff
            si[t, MISSES] += 1
            si[t, LAST] = -1
        si[t, AGE] += 1
        si[t:t + 1, HIST].view(np.uint32)[:] = hist
        if si[t, STATUS] == TENTATIVE and bin(hist & mask_n).count("1") >= p.M:
            si[t, STATUS] = CONFIRMED
        if si[t, STATUS] == TENTATIVE:
            delete = si[t, MISSES] >= p.drop_t or si[t, AGE] >= p.N
        else:
            delete = si[t, MISSES] >= p.drop_c
        if delete:
            sf[t] = 0.0
            si[t] = 0
            dropped += 1
    # 6 start
    free = list(np.flatnonzero(si[:, STATUS] == FREE))
    started = not_started = 0
    for j in np.flatnonzero(valid & (assign == 0)):
        if started == len(free):
            not_started += 1
            continue
        t = free[started]
        started += 1
        meta[0] += 1
        sf[t:t + 1, :3].view(np.int64)[:] = est[j:j + 1].view(np.int64)
        sf[t, 3] = 0.0
        si[t] = (meta[0], CONFIRMED if p.M == 1 else TENTATIVE, 1, 0, 1, 1, j, 0)
        assign[j] = meta[0]
    # 7 record
    meta[1] += 1
    tcount = np.array([int((si[:, STATUS] != FREE).sum()), int((si[:, STATUS] == CONFIRMED).sum()), started, dropped,
                       not_started, int(valid.sum()), matched, 0], np.int32)
    return assign, tcount


def run(state, est, count, p, slot=None, dt=None, slots=None, associate=associate_greedy):
    """A batch applied in place to state = (state_f, state_i, meta).  est [batch][max_hits][3], count
    [batch][2].  Returns (assign [batch][max_hits], snap_f [batch][T][4], snap_i [batch][T][8],
    tcount [batch][8]) as rsp_track_dev writes them."""
    sf, si, meta = state
    est = np.asarray(est, np.float64)
    B, H = est.shape[0], est.shape[1]
    S = sf.shape[0] if slots is None else slots
    T = p.max_tracks
    assign = np.zeros((B, H), np.int32)
    snap_f = np.zeros((B, T, 4), np.float64)
    snap_i = np.zeros((B, T, 8), np.int32)
    tcount = np.zeros((B, 8), np.int32)
    for b in range(B):
        n = min(max(int(count[b][0]), 0), H)
        s = 0 if slot is None else int(slot[b])
        if s < 0 or s >= S:
            e = est[b, :n]
            valid = ~(np.isnan(e[:, 0]) | np.isnan(e[:, 1]))
            assign[b, :n] = np.where(valid, 0, -1)
            tcount[b, N_VALID] = int(valid.sum())
            continue
        a, tc = step(sf[s], si[s], meta[s], est[b], n, p, None if dt is None else dt[b], associate)
        assign[b, :n] = a
        tcount[b] = tc
        snap_f[b].view(np.int64)[:] = sf[s].view(np.int64)
        snap_i[b] = si[s]
    return assign, snap_f, snap_i, tcount


def confirmed(state, slot=0):
    """The confirmed tracks of a slot as a list of dicts (id, r, v, ele, hits, age)."""
    sf, si, _ = state
    return [dict(id=int(si[slot, t, ID]), r=float(sf[slot, t, 0]), v=float(sf[slot, t, 1]), ele=float(sf[slot, t, 2]),
                 hits=int(si[slot, t, HITS]), age=int(si[slot, t, AGE]))
            for t in np.flatnonzero(si[slot, :, STATUS] == CONFIRMED)]


# ------------------------------------------------------------------ scenes
def scene(seed, cpis=60, targets=4, false_alarms=20, max_hits=None, dt=0.08, rate_sign=1.0, pd=0.9, sigma=(3.0, 0.2),
          span=(3000.0, 60.0), nan_plots=0, nan_ele=0.0, quant=None):
    """Constant-velocity targets (500-2500 m, |v| 5-25 m/s, detection probability pd, noise sigma)
    and `false_alarms` uniform false alarms per CPI over span[0] x +-span[1], shuffled.  nan_plots
    plots per CPI get a NaN r or v, a share nan_ele of the plots a NaN ele; quant = (qr, qv) rounds
    the plots to a grid.  The count is the number of plots made, also where max_hits is smaller.
    Returns (est [cpis][max_hits][3], count [cpis][2], truth [cpis][targets][2])."""
    rng = np.random.default_rng(seed)
    r0 = rng.uniform(500.0, 2500.0, targets)
    v0 = rng.uniform(5.0, 25.0, targets) * rng.choice([-1.0, 1.0], targets)
    per = targets + false_alarms + nan_plots
    H = per if max_hits is None else int(max_hits)
    est = np.full((cpis, H, 3), np.nan)       # what lies past the count is never read
    count = np.zeros((cpis, 2), np.int32)
    truth = np.zeros((cpis, targets, 2))
    for b in range(cpis):
        tr = r0 + rate_sign * v0 * dt * b
        truth[b, :, 0], truth[b, :, 1] = tr, v0
        seen = rng.uniform(size=targets) < pd
        rows = [np.stack([tr[seen] + sigma[0] * rng.standard_normal(int(seen.sum())),
                          v0[seen] + sigma[1] * rng.standard_normal(int(seen.sum())),
                          rng.uniform(-5.0, 25.0, int(seen.sum()))], 1),
                np.stack([rng.uniform(0.0, span[0], false_alarms), rng.uniform(-span[1], span[1], false_alarms),
                          rng.uniform(-5.0, 25.0, false_alarms)], 1)]
        if nan_plots:
            bad = np.stack([rng.uniform(0.0, span[0], nan_plots), rng.uniform(-span[1], span[1], nan_plots),
                            rng.uniform(-5.0, 25.0, nan_plots)], 1)
            bad[np.arange(nan_plots), rng.integers(0, 2, nan_plots)] = np.nan
            rows.append(bad)
        p = np.concatenate(rows, 0)
        if quant is not None:
            p[:, 0] = np.round(p[:, 0] / quant[0]) * quant[0]
            p[:, 1] = np.round(p[:, 1] / quant[1]) * quant[1]
        if nan_ele:
            p[rng.uniform(size=len(p)) < nan_ele, 2] = np.nan
        p = p[rng.permutation(len(p))]
        n = min(len(p), H)
        est[b, :n] = p[:n]
        count[b] = (len(p), 0)
    return est, count, truth


def quantised_scene(seed, cpis=16, plots=40, max_hits=48):
    """Plots on a 6 m x 0.5 m/s grid inside a small patch, so equal costs are common: ties between
    tracks for a plot and between plots for a track, and matchings that take several rounds."""
    rng = np.random.default_rng(seed)
    est = np.full((cpis, max_hits, 3), np.nan)
    count = np.zeros((cpis, 2), np.int32)
    for b in range(cpis):
        n = plots if b % 5 != 4 else plots // 2
        est[b, :n, 0] = 1000.0 + 6.0 * rng.integers(0, 12, n)
        est[b, :n, 1] = 0.5 * rng.integers(-3, 4, n)
        est[b, :n, 2] = rng.integers(0, 4, n).astype(np.float64)
        count[b, 0] = n
    return est, count


# ------------------------------------------------------------------ the GPU sweep
# (id, Params, scene keyword arguments or ('quant', seed, cpis, plots, max_hits), d_dt given)
def _p(T, **kw):
    return Params(max_tracks=T, **kw)


CASES = [
    ("t1_p1", _p(1), dict(seed=1, cpis=12, targets=1, false_alarms=0), False),
    ("t5_p0", _p(5), dict(seed=2, cpis=12, targets=0, false_alarms=0, max_hits=4), False),
    ("t5_p63_overflow", _p(5), dict(seed=3, cpis=12, targets=3, false_alarms=60), True),
    ("t64_p64", _p(64), dict(seed=4, cpis=20, targets=4, false_alarms=60, nan_ele=0.2), False),
    ("t65_p65_neg", _p(65, rate_sign=-1.0), dict(seed=5, cpis=20, targets=5, false_alarms=60, rate_sign=-1.0), True),
    ("t256_p300_nan", _p(256), dict(seed=6, cpis=16, targets=8, false_alarms=280, nan_plots=12, nan_ele=0.1), False),
    ("t1024_p1100", _p(1024, gate=(60.0, 4.0)), dict(seed=7, cpis=12, targets=20, false_alarms=1080, max_hits=1024,
                                                      pd=1.0), True),
    ("t64_m1", _p(64, confirm=(1, 1), drop=(1, 2)), dict(seed=8, cpis=14, targets=4, false_alarms=20), False),
    ("t64_n32", _p(64, confirm=(20, 32), drop=(6, 8)), dict(seed=9, cpis=40, targets=4, false_alarms=6, pd=0.8), False),
    ("t64_quant", _p(64, gate=(18.0, 1.0), confirm=(2, 3)), ("quant", 10, 16, 40, 48), False),
    ("t5_quant_overflow", _p(5, gate=(18.0, 1.0), confirm=(2, 3)), ("quant", 11, 12, 40, 41), True),
]


def case_inputs(case):
    """(est, count, dt or None) of a CASES row."""
    _, p, sc, with_dt = case
    if isinstance(sc, tuple):
        est, count = quantised_scene(*sc[1:])
    else:
        est, count, _ = scene(dt=p.dt, **sc)
    dt = None
    if with_dt:   # what a frame clock that is not quite regular gives
        dt = p.dt * (1.0 + 0.25 * np.sin(np.arange(est.shape[0])))
    return est, count, dt


# ------------------------------------------------------------------ the C boundary
def track_params(_capi, max_tracks=64, confirm=(3, 5), drop=(2, 4), reserved=0, dt=0.08, rate_sign=1.0, gate=(30.0, 2.0),
                 alpha=(0.5, 0.5, 0.5)):
    p = _capi.rsp_track_params()
    p.max_tracks, p.confirm_m, p.confirm_n, p.drop_tentative, p.drop_confirmed = max_tracks, confirm[0], confirm[1], \
        drop[0], drop[1]
    p.reserved, p.dt, p.rate_sign, p.gate_r, p.gate_v = reserved, dt, rate_sign, gate[0], gate[1]
    p.alpha_r, p.alpha_v, p.alpha_e = alpha
    return p


# every parameter rsp_track_dev refuses, with a word of its message (the CPU and the GPU test walk it)
BAD_PARAMS = [
    (dict(max_tracks=0), "max_tracks"), (dict(max_tracks=1025), "max_tracks"),
    (dict(confirm=(0, 5)), "confirm"), (dict(confirm=(6, 5)), "confirm"), (dict(confirm=(3, 33)), "confirm"),
    (dict(drop=(0, 4)), "drop"), (dict(drop=(2, 0)), "drop"), (dict(reserved=1), "reserved"),
    (dict(dt=0.0), "dt ="), (dict(dt=-0.08), "dt ="), (dict(dt=float("nan")), "dt ="), (dict(dt=float("inf")), "dt ="),
    (dict(rate_sign=0.0), "rate_sign"), (dict(rate_sign=2.0), "rate_sign"), (dict(rate_sign=float("nan")), "rate_sign"),
    (dict(gate=(0.0, 2.0)), "gate"), (dict(gate=(30.0, -1.0)), "gate"), (dict(gate=(float("nan"), 2.0)), "gate"),
    (dict(gate=(30.0, float("inf"))), "gate"),
    (dict(alpha=(0.0, 0.5, 0.5)), "alpha"), (dict(alpha=(0.5, 1.5, 0.5)), "alpha"), (dict(alpha=(0.5, 0.5, float("nan"))), "alpha"),
]
