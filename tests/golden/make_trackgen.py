"""Writes tests/golden/racing_trackgen.npz from the specification tests/trackgen_ref.py (this project's own restatement; nothing
of the reference runs here):  python tests/golden/make_trackgen.py

64 tracks of one seed, first_track = 0: n_checkpoint, n_tile, attempt, flags, start pose (fp64), start line, boundary and the
crc32 of the fp32 tiles of each; the full fp32 tiles of 8 of them.  The seed is searched (seeds 0, 1, 2, ...) until the 64
hold a winner at attempt 0, a winner at attempt >= R = 16 (so that the kernel's second round of attempts is exercised), a
10-checkpoint and a 19-checkpoint track; what the search found is printed.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import trackgen_ref as R   # noqa: E402

N_TRACKS, N_FULL = 64, 8


def search():
    for seed in range(1000):
        wins = [R.winning_attempt(seed, t) for t in range(N_TRACKS)]
        att = np.array([a for a, _ in wins])
        ncp = np.array([r["n"] if r else 0 for _, r in wins])
        have = dict(first=(att == 0).any(), later=(att >= R.ROUND).any(), ten=(ncp == 10).any(), nineteen=(ncp == 19).any(),
                    none_capped=(att >= 0).all())
        print(f"seed {seed}: attempts max {att.max()} mean {att.mean() + 1:.2f}, winners at 0: {(att == 0).sum()}, at >= {R.ROUND}: "
              f"{(att >= R.ROUND).sum()}, 10 checkpoints: {(ncp == 10).sum()}, 19: {(ncp == 19).sum()}", flush=True)
        if all(have.values()):
            return seed, att, ncp
    raise SystemExit("no seed found")


def main():
    seed, att, ncp = search()
    tracks = [R.build(seed, t) for t in range(N_TRACKS)]
    # the full tiles: one of each kind the search asked for, then the lowest indices
    full = [int(np.flatnonzero(att == 0)[0]), int(np.flatnonzero(att >= R.ROUND)[0]), int(np.flatnonzero(ncp == 10)[0]),
            int(np.flatnonzero(ncp == 19)[0])]
    for t in range(N_TRACKS):
        if len(full) < N_FULL and t not in full and tracks[t]["flags"] == 0:
            full.append(t)
    full = sorted(set(full))
    t = 0
    while len(full) < N_FULL:          # (one track was of two kinds)
        if t not in full and tracks[t]["flags"] == 0:
            full = sorted(full + [t])
        t += 1
    out = dict(seed=np.uint64(seed), n_checkpoint=np.int32([k["n_checkpoint"] for k in tracks]),
               n_tile=np.int32([k["n_tile"] for k in tracks]), attempt=np.int32([k["attempt"] for k in tracks]),
               flags=np.uint32([k["flags"] for k in tracks]), start_pose=np.array([k["start_pose"] for k in tracks]),
               start_line=np.float32([k["start_line"] for k in tracks]), boundary=np.float32([k["boundary"] for k in tracks]),
               crc=np.uint32([R.crc(k["tiles"]) for k in tracks]), start_id=np.int32([k["start_id"] for k in tracks]),
               full=np.int32(full))
    for t in full:
        out[f"tiles_{t}"] = tracks[t]["tiles"]
    path = os.path.join(HERE, "racing_trackgen.npz")
    np.savez_compressed(path, **out)
    print(f"seed {seed}: full tracks {full}, n_tile {out['n_tile'].min()} .. {out['n_tile'].max()}, flags {np.unique(out['flags'])}, "
          f"{os.path.getsize(path)} bytes -> {path}")


if __name__ == "__main__":
    main()
