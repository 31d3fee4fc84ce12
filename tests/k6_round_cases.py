"""The rounds of the gapped stage: a model of k6_pick / k6_resolve (mimeo_amd/csrc/k6_gapped.hip) and seeded pairs for its takes.

TEST INFRASTRUCTURE, beside tests/k6_cases.py.  A round of K6 takes up to `take` anchors of a group (k6_pick), runs their DPs and
replays the ordered skip rule over what exists (k6_resolve).  Which anchors a round takes never changes a record; it changes how many
rounds and how many DP jobs (two per scheduled anchor) a group costs.  `simulate` restates the two kernels for ONE group under the
box rule, from the kernels' text:

* pick: from the group's first unfinalised rank, at most PICK_SCAN ranks, until `take` anchors are scheduled.  An anchor that is not
  NEW is passed over; one inside an accepted box is SKIPPED; one NEAR (<= NEAR_DIAG diagonals and <= NEAR_POS target bases) a pending
  anchor (DP done in an earlier round, not finalised) or one scheduled in this round waits, MAX_DEFER times at most; one that would be
  scheduled beyond the GUARD_FREE-th of the round waits when GUARD_COUNT or more pending or scheduled ones lie within GUARD_DIAG
  diagonals of its own (the guard; it keeps no count of waits); every other one is scheduled.
* resolve: in rank order from the same rank: SKIPPED / ACCEPTED are passed over; an anchor inside a box accepted so far becomes
  SKIPPED, with or without a DP result; a NEW one that is not stops the replay; one with a result is ACCEPTED and adds its box; at
  most RESOLVE_NEW are accepted per invocation.

The model is held to hand-worked cases in tests/test_host_k6_rounds.py and the engine's `[k6] jobs` lines to the model in
tests/test_gpu_k6_rounds.py.  The generators plant copies so that what a round does is known: distinct copies lie more than NEAR_POS
bases and more than GUARD_DIAG diagonals apart from each other, in increasing order on both scaffolds (the chain keeps them all)."""
import numpy as np

from tests import k6_cases as K

# k6_gapped.hip / common.h
OLD_CAP = 32                  # MAX_BATCH of the parent commit: the take under MIMEO_K6_BMAX=32 is the parent's policy
LIMIT = 128                   # MAX_BATCH
ROUND_ANCHORS = 32768         # K6_ROUND_ANCHORS
PICK_SCAN, RESOLVE_NEW = 2048, 256
NEAR_DIAG, NEAR_POS, MAX_DEFER = 256, 8192, 2
GUARD_FREE, GUARD_DIAG, GUARD_COUNT = 32, 4096, 4

NEW, DONE, SKIPPED, ACCEPTED = 0, 1, 2, 3


def default_take(ngroups, env=None):
    """gapped_setup: the round's budget over the groups, at least 1, at most LIMIT; MIMEO_K6_BMAX sets it (same clipping)"""
    t = int(env) if env is not None else ROUND_ANCHORS // ngroups
    return max(1, min(LIMIT, t))


def _relation(a, b):
    dd, dp = abs((a[0] - a[1]) - (b[0] - b[1])), abs(a[0] - b[0])
    return (dd <= NEAR_DIAG and dp <= NEAR_POS), dd <= GUARD_DIAG


def _inside(a, box):
    return box[0] <= a[0] < box[1] and box[2] <= a[1] < box[3]


def simulate(anchors, box_of, take, guard=True, scan=None, max_rounds=100000):
    """anchors: [(t, q)] in rank order; box_of(rank) -> (tstart, tend, qstart, qend) of the alignment that rank's DP gives.
    dict: rounds = rounds that ran a DP (the `[k6] jobs` lines), jobs = [half extensions per such round], accepted = ranks in the
    order they were accepted, wasted = scheduled ranks that were skipped afterwards, invocations = pick / resolve pairs"""
    n, scan = len(anchors), scan or PICK_SCAN
    state, defer = [NEW] * n, [0] * n
    boxes, accepted, jobs, scheduled = [], [], [], []
    nxt = inv = 0
    while True:
        inv += 1
        assert inv <= max_rounds
        # ---- k6_pick
        sb, r = [], nxt
        while r < n and len(sb) < take and r - nxt < scan:
            if state[r] == NEW:
                a = anchors[r]
                if any(_inside(a, b) for b in boxes):
                    state[r] = SKIPPED
                else:
                    others = [anchors[k] for k in range(nxt, r) if state[k] == DONE] + [anchors[k] for k in sb]
                    rel = [_relation(a, b) for b in others]
                    if any(x for x, _ in rel) and defer[r] < MAX_DEFER:
                        defer[r] += 1
                    elif guard and len(sb) >= GUARD_FREE and sum(y for _, y in rel) >= GUARD_COUNT:
                        pass
                    else:
                        sb.append(r)
            r += 1
        for k in sb:
            state[k] = DONE
        scheduled += sb
        if sb:
            jobs.append(2 * len(sb))
        # ---- k6_resolve
        nnew, r = 0, nxt
        while r < n:
            if state[r] not in (SKIPPED, ACCEPTED):
                if nnew == RESOLVE_NEW:
                    break
                if any(_inside(anchors[r], b) for b in boxes):
                    state[r] = SKIPPED
                elif state[r] == NEW:
                    break
                else:
                    boxes.append(tuple(box_of(r)))
                    accepted.append(r)
                    state[r] = ACCEPTED
                    nnew += 1
            r += 1
        nxt = r
        if nxt >= n:
            break
    return dict(rounds=len(jobs), jobs=jobs, accepted=accepted, wasted=[k for k in scheduled if state[k] != ACCEPTED], invocations=inv)


# ------------------------------------------------------------------------------------------------ seeded pairs
STEP_T, STEP_Q = 13400, 9100     # between distinct copies: > NEAR_POS + the longest copy on both scaffolds, diagonals STEP_T - STEP_Q > GUARD_DIAG apart
assert STEP_Q > NEAR_POS + 800 and STEP_T - STEP_Q > GUARD_DIAG


def distinct_pairs(n, seed):
    """two scaffolds with n planted copy pairs of 400-800 bases at 90 % identity (substitutions only), copy i at target 1000 + i STEP_T
    and query 1000 + i STEP_Q.  Returns (T, Q, [(t, q, length)])"""
    rng = np.random.default_rng(seed)
    T, Q = K.rand(rng, 2000 + n * STEP_T), K.rand(rng, 2000 + n * STEP_Q)
    plan = []
    for i in range(n):
        ln = int(rng.integers(400, 801))
        core = K.rand(rng, ln)
        t, q = 1000 + i * STEP_T, 1000 + i * STEP_Q
        T[t:t + ln] = core
        Q[q:q + ln] = K.substitute(rng, core, 0.10)
        plan.append((t, q, ln))
    return T.tobytes(), Q.tobytes(), plan


def collinear_pair(length, seed, sub=0.12, indel_every=900, flank=20000):
    """one copy of `length` bases at 88 % identity with an indel of 1-3 bases about every `indel_every` bases, between random flanks:
    one alignment, and a chained HSP per gap-free stretch"""
    rng = np.random.default_rng(seed)
    core = K.rand(rng, length)
    copy = K.substitute(rng, core, sub)
    at = np.sort(rng.choice(np.arange(200, length - 200), size=length // indel_every, replace=False))
    indels = [(int(p), int(k)) for p, k in zip(at, rng.choice([-3, -2, -1, 1, 2, 3], size=at.size))]
    copy = K.with_indels(rng, copy, indels)
    T = np.concatenate([K.rand(rng, flank), core, K.rand(rng, flank)])
    Q = np.concatenate([K.rand(rng, flank + 3000), copy, K.rand(rng, flank)])
    return T.tobytes(), Q.tobytes()


def fragmented_pairs(ncopies, nsmall, seed, length=12000, indel_every=350):
    """what a row of the benchmark's genome looks like to k6_pick: `ncopies` long copies that the gap-free stage leaves as some twenty
    HSPs each (an indel of 1-3 bases about every `indel_every` bases), so that the chain is longer than the 512 ranks the window used
    to hold, and `nsmall` identical copies of 50-61 bases whose single HSP ranks among the shortest fragments, beyond rank 512.  Copies in increasing order on both
    scaffolds, distinct ones apart as in distinct_pairs"""
    rng = np.random.default_rng(seed)
    T, Q = [K.rand(rng, 1000)], [K.rand(rng, 1000)]
    for i in range(ncopies + nsmall):
        ln = length if i < ncopies else int(rng.integers(50, 62))
        core = K.rand(rng, ln)
        copy = K.substitute(rng, core, 0.10) if ln == length else core.copy()
        if ln == length:
            at = rng.choice(np.arange(100, ln - 100), size=ln // indel_every, replace=False)
            copy = K.with_indels(rng, copy, [(int(p), int(k)) for p, k in zip(at, rng.choice([-3, -2, -1, 1, 2, 3], size=at.size))])
        T += [core, K.rand(rng, STEP_T)]
        Q += [copy, K.rand(rng, STEP_Q)]
    return np.concatenate(T).tobytes(), np.concatenate(Q).tobytes()


def near_miss_pair(seed, apart=2000, diagonals=100, length=600):
    """two copy pairs `apart` target bases and `diagonals` diagonals from each other: NEAR, so the lower-ranked waits for the other's
    DP, and far enough that the other's alignment (the copy and what the y-drop lets it run into random flanks) does not hold it"""
    rng = np.random.default_rng(seed)
    T, Q = K.rand(rng, 30000), K.rand(rng, 30000)
    for t, q in ((10000, 12000), (10000 + apart, 12000 + apart - diagonals)):
        core = K.rand(rng, length)
        T[t:t + length] = core
        Q[q:q + length] = K.substitute(rng, core, 0.10)
    return T.tobytes(), Q.tobytes()


# ------------------------------------------------------------------------------------------------ the oracle's view of a pair
def ranked_anchors(T, Q):
    """plus strand: the anchors of the oracle's chained HSPs in anchor order (score descending, tstart, qstart, length)"""
    from oracle import oracle as O
    h = O.ungapped_hsps(T, Q, 0, O.default_params())
    h = h[(h['flags'] & 1) == 1]
    h = h[np.lexsort((h['length'], h['qstart'], h['tstart'], -h['score']))]
    out = []
    for x in h:
        off = K.best_window(T, Q, int(x['tstart']), int(x['qstart']), int(x['length']))
        out.append((int(x['tstart']) + off, int(x['qstart']) + off))
    return out


def predict(anchors, exp, take, guard=True, scan=None):
    """simulate() on a pair: anchors = ranked_anchors(T, Q), the box of an anchor = the one alignment of `exp` (the oracle's
    plus-strand records) that holds it"""
    rows = [(int(e['tstart']), int(e['tend']), int(e['qstart']), int(e['qend'])) for e in exp]

    def box_of(r):
        hold = [b for b in rows if _inside(anchors[r], b)]
        assert len(hold) == 1, (r, anchors[r], hold)
        return hold[0]
    return simulate(anchors, box_of, take, guard=guard, scan=scan)
