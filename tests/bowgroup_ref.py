"""TEST INFRASTRUCTURE: a restatement, with dicts keyed by frame index and Python floats (IEEE doubles), of the GROUPING between the BoW scores and the
candidates in MapUser::Relocalization (src/map_user.cc:177-270, 331, 347-363) and MapRefiner::LoopDetection (src/map_refiner.cc:132-214).  It follows the
reference statement by statement, not the kernel's data layout; include/airfe.h ("Grouping") states the same contract for the device.

The two stated differences are the contract's: every std::map / std::set iteration is in ascending frame index (the reference's is in pointer order), and
the final sort breaks ties to the lower frame index (std::sort is not stable)."""
import math

OK, NO_GROUP, OVERFLOW = 0, 1, 2
RELOC, LOOP = 0, 1


def covis_dict(row_ptr, nbr, weight):
    """CSR -> frame -> [(neighbour, weight)] in the table's order = GetConnectedFrames' map, the frame's own entry included as the table has it"""
    return {f: [(int(nbr[e]), int(weight[e])) for e in range(row_ptr[f], row_ptr[f + 1])] for f in range(len(row_ptr) - 1)}


def _stored_groups(frame_scores, covis):
    """map_user.cc:177-217 ≡ map_refiner.cc:132-172 -> (group_candidates: deputy -> (group_frames set, group_score), best_group_score)"""
    group_candidates = {}
    best_group_score = -1.0
    for fsw in sorted(frame_scores):                                   # for(; fs_it != frame_scores.end(); fs_it++)
        deputy_of_group = fsw
        deputy_score = frame_scores[fsw]
        group_frames = {fsw}
        group_score = 0.0
        group_score += deputy_score
        for covi_frame, w in sorted(covis.get(fsw, ())):                # for(auto& kv : fsw_covi_frames)
            if w > 10 and covi_frame in frame_scores:
                covi_score = frame_scores[covi_frame]
                group_frames.add(covi_frame)
                group_score += covi_score
                if covi_score > deputy_score:
                    deputy_of_group = covi_frame
                    deputy_score = covi_score
        if deputy_of_group not in group_candidates or group_candidates[deputy_of_group][1] < group_score:
            group_candidates[deputy_of_group] = (group_frames, group_score)
            if group_score > best_group_score:
                best_group_score = group_score
    return group_candidates, best_group_score


def _ranked(scores, K):
    """descending score, ties to the lower frame index -> (frames [K] -1 padded, scores [K] 0.0 padded)"""
    order = sorted(scores, key=lambda f: (-scores[f], f))[:K]
    return order + [-1] * (K - len(order)), [scores[f] for f in order] + [0.0] * (K - len(order))


def group(mode, cands, covis, K, ccap=None, ncand=None, extra=None, positions=None, qpos=None, max_dist=None):
    """cands: [(frame, score)] ascending in frame = frame_scores; covis: covis_dict's; extra: frame -> junction term or None; positions: frame -> (x, y, z)
    -> dict(frames [K], scores [K], ngroups, status)"""
    none = dict(frames=[-1] * K, scores=[0.0] * K, ngroups=0)
    ncand = len(cands) if ncand is None else ncand
    if ccap is not None and ncand > ccap:
        return dict(none, status=OVERFLOW)
    frame_scores = {int(f): float(s) for f, s in cands}
    group_candidates, best_group_score = _stored_groups(frame_scores, covis)
    if best_group_score < 0:
        return dict(none, status=NO_GROUP)
    scores = {}
    if mode == RELOC:
        best_group_score = 0.0                                         # map_user.cc:223
        for deputy in sorted(group_candidates):
            group_scores = [frame_scores[f] for f in sorted(group_candidates[deputy][0])]
            if len(group_scores) > 5:
                group_scores.sort(reverse=True)
            total = 0.0
            for v in group_scores[:5]:
                total += v
            scores[deputy] = total
            best_group_score = max(best_group_score, total)
        if len(scores) > 3:
            thr = best_group_score * 0.5
            scores = {d: s for d, s in scores.items() if not s < thr}
        if extra is not None:
            scores = {d: s + float(extra[d]) for d, s in scores.items()}      # kv.second.group_score += junction_frame_scores * (1 + rate)
    else:
        for deputy in sorted(group_candidates):
            scores[deputy] = group_candidates[deputy][1]
            dx, dy, dz = (float(qpos[k]) - float(positions[deputy][k]) for k in range(3))
            if math.sqrt((dx * dx + dy * dy) + dz * dz) > max_dist:
                del scores[deputy]
        if len(scores) > 3:
            thr = best_group_score * 0.5
            scores = {d: s for d, s in scores.items() if not s < thr}
    frames, top = _ranked(scores, K)
    return dict(frames=frames, scores=top, ngroups=len(scores), status=OK)
