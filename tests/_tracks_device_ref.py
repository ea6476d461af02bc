"""Restatement of ssfm_build_tracks_device (include/ssfm.h) in numpy / plain Python, and the helpers its tests share: seeded scenes, the flat arrays of the
C call, and the relabelling of a host build_tracks(..., merge=True) result to canonical ids.  Test infrastructure only."""
import numpy as np


def flatten(features, image_matches):
    """lists -> (fptr, fxy, i0, i1, mptr, f0, f1) exactly as given: nothing sorted, nothing made unique"""
    K = len(features)
    fptr = np.zeros(K + 1, np.int32)
    fptr[1:] = np.cumsum([len(f) for f in features])
    fxy = np.concatenate([np.asarray(f, np.float64).reshape(-1, 2) for f in features]) if fptr[-1] else np.zeros((0, 2))
    i0 = np.array([m[0] for m in image_matches], np.int32); i1 = np.array([m[1] for m in image_matches], np.int32)
    mptr = np.zeros(len(image_matches) + 1, np.int32)
    mptr[1:] = np.cumsum([len(m[2]) for m in image_matches])
    pairs = np.array([p for m in image_matches for p in m[2]], np.int32).reshape(-1, 2)
    return fptr, fxy, i0, i1, mptr, pairs[:, 0].copy(), pairs[:, 1].copy()


def components(fptr, fxy, i0, i1, mptr, f0, f1, centerx=0.0, centery=0.0):
    """The definitions of the header, by a plain union-find: tracks, canonical ids, winners, conflicts, output order."""
    fptr = np.asarray(fptr, np.int64); total = int(fptr[-1])
    parent = list(range(total)); touched = np.zeros(total, bool)

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for s in range(len(i0)):
        a, b = int(i0[s]), int(i1[s])
        for m in range(int(mptr[s]), int(mptr[s + 1])):
            assert 0 <= f0[m] < fptr[a + 1] - fptr[a] and 0 <= f1[m] < fptr[b + 1] - fptr[b]
            g0, g1 = int(fptr[a] + f0[m]), int(fptr[b] + f1[m])
            touched[g0] = touched[g1] = True
            r0, r1 = find(g0), find(g1)
            if r0 != r1:
                parent[max(r0, r1)] = min(r0, r1)
    root = np.array([find(g) for g in range(total)], np.int64) if total else np.zeros(0, np.int64)
    smallest = {}                                                  # component -> its smallest member (whatever the union-find made of its roots)
    for g in np.flatnonzero(touched):
        smallest.setdefault(int(root[g]), int(g))                  # g ascends: the first seen is the smallest
    order = sorted(smallest.values())
    ident = {int(root[g]): k for k, g in enumerate(order)}
    tracks = np.full(total, -1, np.int32)
    for g in np.flatnonzero(touched):
        tracks[g] = ident[int(root[g])]
    cam_of = np.searchsorted(fptr, np.arange(total), side="right") - 1 if total else np.zeros(0, np.int64)
    P = len(order)
    winner = {}; conflict = np.zeros(P, bool)
    for g in np.flatnonzero(touched):                              # ascending g: the first on a key wins, a second one flags the track
        key = (int(cam_of[g]), int(tracks[g]))
        if key in winner:
            conflict[key[1]] = True
        else:
            winner[key] = int(g)
    gs = np.array(sorted(winner.values()), np.int64)
    fxy = np.asarray(fxy, np.float64).reshape(-1, 2)
    return dict(tracks=tracks, num_points=P, conflict=conflict, obs_cam=cam_of[gs].astype(np.int32), obs_pt=tracks[gs].astype(np.int32),
                obs_feat=(gs - fptr[cam_of[gs]]).astype(np.int32), obs_xy=fxy[gs] - np.array([centerx, centery]) if len(gs) else np.zeros((0, 2)))


def relabel_host(host, fptr):
    """A build_tracks(..., merge=True) result in canonical ids: every alive track is renamed by the rank of its smallest member.
    -> dict(tracks [total], num_points (alive ids), keys {(camera, canonical id): (x, y)}, members {(camera, canonical id): number of features})"""
    flat = np.concatenate([np.asarray(t, np.int64) for t in host["tracks"]]) if len(host["tracks"]) else np.zeros(0, np.int64)
    first = {}
    for g in np.flatnonzero(flat >= 0):
        first.setdefault(int(flat[g]), int(g))
    ident = {t: k for k, (t, _) in enumerate(sorted(first.items(), key=lambda kv: kv[1]))}
    tracks = np.array([ident[int(t)] if t >= 0 else -1 for t in flat], np.int32)
    keys = {(int(c), ident[int(p)]): (float(xy[0]), float(xy[1])) for c, p, xy in zip(host["obs_cam"], host["obs_pt"], host["obs_xy"])}
    cam_of = np.searchsorted(np.asarray(fptr, np.int64), np.arange(len(flat)), side="right") - 1
    members = {}
    for g in np.flatnonzero(tracks >= 0):
        k = (int(cam_of[g]), int(tracks[g])); members[k] = members.get(k, 0) + 1
    assert int(np.count_nonzero(host["alive"])) == len(ident)
    return dict(tracks=tracks, num_points=len(ident), keys=keys, members=members)


def device_keys(dev):
    """{(camera, track): (x, y)} of a device (or restated) result"""
    return {(int(c), int(p)): (float(xy[0]), float(xy[1])) for c, p, xy in zip(dev["obs_cam"], dev["obs_pt"], dev["obs_xy"])}


def scene(num_frames, num_features, num_points, pairs, wrong_frac=0.0, seed=0, shuffle=True, max_matches=None):
    """Frames that each see num_features of num_points world points (a point at most once per frame: the true matches are conflict-free); a match set per
    frame pair holds the points both see, wrong_frac of them re-pointed at a random feature.  Shuffled sets start many tracks apart that merge later.
    -> (features, image_matches) in the list form of tracks.build_tracks, every set in ascending first index with unique first indices."""
    rng = np.random.default_rng(seed)
    seen = [rng.permutation(num_points)[:num_features] for _ in range(num_frames)]            # feature j of frame k shows point seen[k][j]
    where = []
    for k in range(num_frames):
        w = np.full(num_points, -1, np.int64); w[seen[k]] = np.arange(num_features); where.append(w)
    features = [rng.uniform(0.0, 1000.0, (num_features, 2)) for _ in range(num_frames)]
    image_matches = []
    for a, b in pairs:
        both = np.flatnonzero((where[a] >= 0) & (where[b] >= 0))
        if max_matches is not None and len(both) > max_matches:
            both = np.sort(rng.choice(both, max_matches, replace=False))
        fa, fb = where[a][both], where[b][both].copy()
        wrong = rng.random(len(fb)) < wrong_frac
        fb[wrong] = rng.integers(0, num_features, int(wrong.sum()))
        o = np.argsort(fa)
        image_matches.append((int(a), int(b), list(zip(fa[o].tolist(), fb[o].tolist()))))
    if shuffle:
        image_matches = [image_matches[i] for i in rng.permutation(len(image_matches))]
    return features, image_matches


def chain_pairs(num_frames, reach, extra=0, seed=0):
    """(i, i + d), d = 1 .. reach, plus `extra` random other pairs"""
    pairs = [(i, i + d) for d in range(1, reach + 1) for i in range(num_frames - d)]
    rng = np.random.default_rng(seed)
    have = set(pairs)
    while extra > 0:
        a, b = sorted(rng.choice(num_frames, 2, replace=False).tolist())
        if (a, b) not in have:
            have.add((a, b)); pairs.append((a, b)); extra -= 1
    return pairs
