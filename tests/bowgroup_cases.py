"""TEST INFRASTRUCTURE: the grouping cases the CPU and the GPU suites share (tests/test_bowgroup_cpu.py, tests/test_gpu_reloc.py): seeded random cases and
constructed ones, each built to contain one of the situations include/airfe.h ("Grouping") distinguishes.  Scores of the constructed cases are dyadic
rationals, so that sums, halves and ties are exact by construction."""
import numpy as np

import bowgroup_ref as gr


def csr(N, rows):
    """rows: frame -> [(neighbour, weight)] -> (row_ptr [N + 1], nbr, weight) int32, every row ascending in neighbour"""
    row_ptr, nbr, weight = [0], [], []
    for f in range(N):
        for n, w in sorted(rows.get(f, ())):
            nbr.append(n)
            weight.append(w)
        row_ptr.append(len(nbr))
    return np.array(row_ptr, np.int32), np.array(nbr, np.int32), np.array(weight, np.int32)


def case(name, mode, N, cands, rows, K=None, ccap=None, ncand=None, extra=None, positions=None, qpos=(0.0, 0.0, 0.0), max_dist=1e300):
    K = K or (3 if mode == gr.RELOC else 5)
    cands = sorted((int(f), float(s)) for f, s in cands)
    row_ptr, nbr, weight = csr(N, rows)
    pos = np.zeros((N, 3)) if positions is None else np.asarray(positions, np.float64)
    return dict(name=name, mode=mode, N=N, cands=cands, row_ptr=row_ptr, nbr=nbr, weight=weight, K=K, ccap=ccap or max(len(cands), 1),
                ncand=len(cands) if ncand is None else ncand, extra=None if extra is None else np.asarray(extra, np.float64), positions=pos,
                qpos=np.asarray(qpos, np.float64), max_dist=float(max_dist))


def random_case(seed, mode, N=None, ncand=None):
    """40-300 frames, 0-200 candidates, a sparse covisibility among nearby frames with weights 1-40 and the frames' own entries; a quarter of the cases
    draw their scores from 32 dyadic values, so that equal scores and equal sums occur"""
    rng = np.random.default_rng(seed)
    N = int(rng.integers(40, 301)) if N is None else N
    ncand = int(rng.integers(0, min(N, 200) + 1)) if ncand is None else ncand
    frames = np.sort(rng.choice(N, size=ncand, replace=False))
    scores = rng.integers(1, 33, ncand) / 64.0 if seed % 4 == 0 else rng.uniform(0.01, 0.5, ncand)
    rows = {}
    for f in range(N):
        deg = int(rng.integers(0, 13))
        near = set(int(x) for x in np.clip(f + rng.integers(-15, 16, deg), 0, N - 1))
        near.discard(f)
        if rng.random() < 0.7:
            near.add(f)
        rows[f] = [(n, int(rng.integers(1, 41))) for n in near]
    extra = rng.integers(0, 17, N) / 64.0 if (mode == gr.RELOC and seed % 3 == 0) else None
    positions = rng.integers(-6, 7, (N, 3)).astype(np.float64)
    return case(f"random{seed}", mode, N, zip(frames, scores), rows, extra=extra, positions=positions, qpos=(0.0, 1.0, 0.0),
                max_dist=float(rng.integers(3, 9)))


def constructed():
    R, L = gr.RELOC, gr.LOOP
    out = []
    # the frame's own entry above and below the weight floor; a deputy that is not the candidate itself
    out.append(case("self_entries", R, 40, [(3, 8 / 64), (5, 20 / 64), (9, 12 / 64), (11, 6 / 64)],
                    {3: [(3, 20), (5, 25)], 5: [(5, 10), (3, 11)], 9: [(9, 11)], 11: [(11, 3), (12, 40)]}))
    # two candidates electing the same deputy: the second's score larger (deputy 10), equal (deputy 20), smaller (deputy 30)
    out.append(case("same_deputy", R, 40, [(4, 4 / 64), (6, 6 / 64), (10, 32 / 64), (14, 5 / 64), (16, 5 / 64), (20, 30 / 64), (24, 7 / 64), (26, 3 / 64),
                                           (30, 28 / 64)],
                    {4: [(10, 20)], 6: [(10, 20)], 14: [(20, 12)], 16: [(20, 12)], 24: [(30, 40)], 26: [(30, 40)]}))
    # groups of exactly 5, of 6 and of 9 members — the last with equal scores among its top five
    rows = {2: [(n, 20) for n in (2, 3, 4, 5, 6)], 12: [(n, 20) for n in (10, 11, 13, 14, 15)], 25: [(n, 20) for n in range(21, 30) if n != 25]}
    cands = [(2, 9 / 64), (3, 1 / 64), (4, 2 / 64), (5, 3 / 64), (6, 4 / 64)]
    cands += [(10, 1 / 64), (11, 2 / 64), (12, 8 / 64), (13, 3 / 64), (14, 4 / 64), (15, 5 / 64)]
    cands += [(21, 4 / 64), (22, 4 / 64), (23, 1 / 64), (24, 4 / 64), (25, 10 / 64), (26, 4 / 64), (27, 2 / 64), (28, 4 / 64), (29, 3 / 64)]
    out.append(case("members_5_6_9", R, 40, cands, rows))
    # exactly 3 and exactly 4 stored groups, on either side of the `> 3` filter; a group exactly at best * 0.5 stays, one below goes
    out.append(case("three_groups", R, 40, [(1, 32 / 64), (7, 4 / 64), (9, 16 / 64)], {}))
    out.append(case("four_groups", R, 40, [(1, 32 / 64), (7, 4 / 64), (9, 16 / 64), (30, 15 / 64)], {}))
    out.append(case("four_groups_loop", L, 40, [(1, 32 / 64), (7, 4 / 64), (9, 16 / 64), (30, 15 / 64)], {}))
    # equal final scores: the lower frame index first
    out.append(case("ties", R, 40, [(31, 16 / 64), (2, 16 / 64), (17, 16 / 64), (8, 16 / 64), (20, 20 / 64)], {}))
    out.append(case("ties_loop", L, 40, [(31, 16 / 64), (2, 16 / 64), (17, 16 / 64), (8, 16 / 64), (20, 20 / 64), (5, 16 / 64), (6, 16 / 64)], {}))
    # the junction term reorders the top 3 (and lifts a group that was fourth)
    extra = np.zeros(40)
    extra[12], extra[3] = 24 / 64, 2 / 64
    out.append(case("extra", R, 40, [(3, 30 / 64), (6, 28 / 64), (9, 26 / 64), (12, 20 / 64), (15, 18 / 64)], {}, extra=extra))
    # no candidate; more candidates than the list holds
    out.append(case("empty", R, 40, [], {}))
    out.append(case("empty_loop", L, 40, [], {}))
    out.append(case("overflow", R, 40, [(f, (f + 1) / 64) for f in range(8)], {}, ccap=8, ncand=9))
    # every score negative: best_group_score stays below 0
    out.append(case("negative", R, 40, [(2, -2.0), (5, -3.0)], {2: [(5, 20)]}))
    # the loop form: a deputy exactly at max_dist stays, one a hair beyond goes — and the 0.5 filter still uses the best score of a group the distance
    # filter dropped (31/64: 15/64 and below go; with the best of the groups left, 18/64, nothing would); every group beyond
    pos = np.zeros((40, 3))
    pos[4], pos[8], pos[12], pos[16] = (3, 4, 0), (3, 4, 0.5), (0, 5, 0), (0, 0, 5.0000000001)
    out.append(case("loop_exact", L, 40, [(4, 10 / 64), (8, 30 / 64), (12, 12 / 64), (16, 31 / 64), (20, 9 / 64), (24, 15 / 64)], {20: [(20, 30)]}, positions=pos, max_dist=5.0))
    pos = np.full((40, 3), 9.0)
    out.append(case("loop_all_beyond", L, 40, [(4, 10 / 64), (8, 30 / 64), (12, 12 / 64)], {}, positions=pos, max_dist=5.0))
    return out


def all_cases():
    out = constructed()
    out += [random_case(s, gr.RELOC) for s in range(1, 13)]
    out += [random_case(100 + s, gr.LOOP) for s in range(1, 9)]
    # more candidates than two waves of lanes hold (the kernel's per-candidate pass strides over 256 lanes, 64 to a wave)
    out.append(dict(random_case(777, gr.RELOC, N=200, ncand=130), name="wide130"))
    return out


def reference(c):
    """the restatement's answer for a case"""
    covis = gr.covis_dict(c["row_ptr"], c["nbr"], c["weight"])
    return gr.group(c["mode"], c["cands"], covis, c["K"], ccap=c["ccap"], ncand=c["ncand"],
                    extra=None if c["extra"] is None else {f: c["extra"][f] for f in range(c["N"])},
                    positions={f: c["positions"][f] for f in range(c["N"])}, qpos=c["qpos"], max_dist=c["max_dist"])
