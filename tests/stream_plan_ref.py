"""Which points every wave of a stream-kernel launch adds up, restated in Python (tests/test_stream_plan_ref_cpu.py holds it to the library's own plan,
tests/test_stream_edges_gpu.py takes its geometries from CASES).  A helper, not a test.

Restates make_stream_plan (csrc/gp_vgicp_plan.hpp), plan_tile and split_tile (csrc/gp_vgicp_shared.hpp) and the fixed tiles of a factor below the planning
threshold (build_table, csrc/gp_vgicp_table.hip).  Written as lists of per-workgroup chunk counts and running sums, not as the closed forms the kernel evaluates:
  * the n // 64 full chunks go to the 8 XCDs in proportion to their weights (whole chunks, largest remainders first);
  * an XCD's gx workgroups come in dispatch rounds of 32: a workgroup of round r in front of the last takes ceil(mean * (1 + skew * ((rounds - 1) / 2 - r))) chunks,
    the last round shares what is left as evenly as it goes (the first ones one more).  A skew that would leave a last round nothing, or less than a third of the
    mean share per workgroup, is refused: every XCD is then dealt flat;
  * a workgroup's chunks go to its four waves as evenly as they go (the first ones one more); the n % 64 points behind the last full chunk belong to the last
    wave of the last workgroup.
The floating-point expressions are those of the C++ (IEEE doubles, same order), so that a half-way case rounds the same way."""
import math

import numpy as np

NUM_XCD, CHUNK, ROUND, WAVES = 8, 64, 32, 4
RESIDENT_WORKGROUPS = 1024
PLAN_MIN_POINTS = 65536  # kPlanMinPoints: single factors from here on are planned
AUTO_SKEW = 150
XCD_WEIGHT_PERMILLE = (1090, 1070, 1045, 1025, 905, 935, 950, 980)  # kXcdWeightPermille, measured at 15.26 chunks per workgroup


def _lround(x):
    return int(math.floor(x + 0.5)) if x >= 0 else -int(math.floor(-x + 0.5))


def _even(total, parts):
    """`total` items over `parts` holders as evenly as they go, the first ones one more"""
    return [total // parts + (1 if k < total % parts else 0) for k in range(parts)]


def xcd_shares(chunks, weights):
    w = [max(int(v), 1) for v in weights]
    wsum = sum(w)
    share = [chunks * v // wsum for v in w]
    frac = [chunks * v % wsum for v in w]
    for _ in range(chunks - sum(share)):
        best = max(range(NUM_XCD), key=lambda x: (frac[x], -x))  # the first of equals
        share[best] += 1
        frac[best] = -1
    return share


def stream_plan(n, max_workgroups=RESIDENT_WORKGROUPS, skew=-1, weights=None):
    """-> dict(workgroups G, gx, skewed, last_begin, chunks [8][gx] = full chunks of every workgroup, XCD-major)"""
    C = n // CHUNK
    cap = max(NUM_XCD, min(max_workgroups, RESIDENT_WORKGROUPS) // NUM_XCD * NUM_XCD)
    need = -(-max(-(-C // WAVES), 1) // NUM_XCD) * NUM_XCD  # one chunk per wave at least, where there are that many
    G = min(cap, need)
    gx = G // NUM_XCD
    if skew < 0:
        skew = AUTO_SKEW
    if weights is None:
        k = min(2.0, 15.26 / max(C / G, 1.0))
        weights = [1000 + _lround((v - 1000) * k) for v in XCD_WEIGHT_PERMILLE]
    share = xcd_shares(C, weights)
    rounds = -(-gx // ROUND)
    late = gx - ROUND * (rounds - 1)  # workgroups of the last round
    early = None
    if skew > 0 and rounds > 1:
        early = []
        for x in range(NUM_XCD):
            mean = share[x] / gx
            per_round = [max(0, int(math.ceil(mean * (1.0 + (skew / 1000.0) * (0.5 * (rounds - 1) - r)) - 1e-9))) for r in range(rounds - 1)]
            rest = share[x] - ROUND * sum(per_round)
            if rest < 0 or rest * 3 * gx < share[x] * late:
                early = None
                break
            early.append((per_round, rest))
    chunks = []
    for x in range(NUM_XCD):
        if early is None:
            chunks.append(_even(share[x], gx))
        else:
            per_round, rest = early[x]
            chunks.append([c for c in per_round for _ in range(ROUND)] + _even(rest, late))
    return dict(workgroups=G, gx=gx, skewed=early is not None, last_begin=ROUND * (rounds - 1) if early is not None else 0, chunks=chunks, share=share)


def _waves_of(begin, count):
    """(first point, full chunks, tail) of the four waves of a workgroup that owns [begin, begin + count)"""
    out, first = [], begin
    for w, c in enumerate(_even(count // CHUNK, WAVES)):
        out.append((first, c, count % CHUNK if w == WAVES - 1 else 0))
        first += c * CHUNK
    return out


def planned_tiles(n, max_workgroups=RESIDENT_WORKGROUPS, skew=-1, weights=None):
    """-> (plan, tiles [G][2] = first point and points of every workgroup in tile-list order (XCD-major))"""
    p = stream_plan(n, max_workgroups, skew, weights)
    tiles, at = [], 0
    for x in range(NUM_XCD):
        for c in p["chunks"][x]:
            tiles.append([at, c * CHUNK])
            at += c * CHUNK
    tiles[-1][1] += n % CHUNK
    return p, np.array(tiles, dtype=np.int64).reshape(-1, 2)


def fixed_tiles(n, tile_points):
    assert tile_points > 0 and tile_points % (WAVES * CHUNK) == 0
    return np.array([[b, min(tile_points, n - b)] for b in range(0, n, tile_points)], dtype=np.int64).reshape(-1, 2)


def waves(tiles):
    """[len(tiles) * 4][3]: first point, full chunks, tail of every wave"""
    return np.array([w for b, c in tiles.tolist() for w in _waves_of(b, c)], dtype=np.int64).reshape(-1, 3)


def launch_waves(n, max_workgroups=RESIDENT_WORKGROUPS, skew=-1, weights=None, tile_points=0):
    """the waves of the launch a single factor of n points gets: planned (tile_points == 0) or on fixed tiles"""
    if tile_points:
        return None, waves(fixed_tiles(n, tile_points))
    p, tiles = planned_tiles(n, max_workgroups, skew, weights)
    return p, waves(tiles)


def _w(**kw):
    w = [1000] * NUM_XCD
    for x, v in kw.items():
        w[int(x[1:])] = v
    return tuple(w)


# The geometries of tests/test_stream_edges_gpu.py: (n, workgroup cap, GP_TUNE_BALANCE, XCD weights or None = the library's table).  A planned launch needs
# n >= PLAN_MIN_POINTS; C = n // 64 chunks.
N_CONTROL = 65_535        # one below the threshold: fixed tiles
N_MIN = (65_536, 65_537, 65_599)  # C = 1024, tails 0 / 1 / 63
N_LONG = 131_072          # C = 2048: 64 chunks per wave at 8 workgroups
N_MID = (140_011, 163_903, 196_607)  # C = 2187 / 2560 / 3071 at 256 workgroups: 8.5 - 12 chunks per workgroup = 2 - 3 per wave; tails 43 / 63 / 63
N_SKEW_MIN = 67_429       # C = 1053: 264 workgroups at the default cap, gx = 33 = one full round + a last round of ONE workgroup per XCD; tail 37
N_SKEW_DEF = 120_925      # C = 1889: 480 workgroups at the default cap, gx = 60 = one full round + a last round of 28; tail 29
N_SKEW = 198_719          # C = 3104: 776 workgroups at the default cap, gx = 97 = three full rounds + a last round of one; tail 63
BALANCES = (0, 50, 150, 400, 1000)
CAPS = (8, 16, 64, 256, 1024)
# Which of these the plan deals skewed (stream_plan()["skewed"]; tests/test_stream_plan_ref_cpu.py asserts each statement).  The early rounds' shares are rounded UP, so a
# skew is accepted only where the last round has enough workgroups to absorb that: at the default cap
#   * N_SKEW_DEF (gx = 60) takes 50, 150 and 400 (two rounds); 1000 overdraws and is refused;
#   * N_MID[2] = 196,607 (gx = 96) takes 50 and 150 (three rounds, a full last one); 400 is refused;
#   * N_SKEW_MIN (gx = 33) and N_SKEW (gx = 97), each with ONE workgroup in the last round, refuse every value of BALANCES: five times the same flat plan each,
#     the device side of "refused".  With one late workgroup a skew s needs 33 mean - 32 ceil(mean (1 + s / 2)) >= mean / 3, i.e. s <= 41 per mille.
# The smallest skewed plan, gx = 33 with last_begin = 32, therefore runs at balance 40: N_SKEW under a cap of 264 with equal XCD weights, 12 chunks per early
# workgroup and 4 in the single late one.  Further skewed plans of N_SKEW under a cap: 304 at 50 (gx = 38), 512 (gx = 64, two full rounds: takes every value,
# 1000 included), 728 and 768 (three rounds, gx = 91 / 96).  Four skewed rounds need gx >= 97 with more than ~6 chunks per workgroup: 400 k points and up, which
# tests/test_vgicp_gpu.py runs.
SKEWED_CAPS = [(304, 50), (728, 150), (768, 50), (768, 150)] + [(512, bal) for bal in BALANCES]
CASES = (
    [(n, cap, -1, None) for n in N_MIN for cap in CAPS]
    + [(N_LONG, 8, -1, None)]
    + [(n, 256, -1, None) for n in N_MID]
    + [(n, 1024, bal, None) for n in (N_SKEW_MIN, N_SKEW_DEF, N_SKEW) for bal in BALANCES]
    + [(N_MID[2], 1024, bal, None) for bal in (0, 50, 150, 400)]
    + [(N_SKEW, 264, 40, (1000,) * NUM_XCD)]
    + [(N_SKEW, cap, bal, None) for cap, bal in SKEWED_CAPS]
    # one XCD at 500 and another at 1500 (the ends of GP_TUNE_XCD_WEIGHT_x): the one's workgroups get half the mean share, the other's one and a half
    + [(65_599, 1024, -1, _w(x2=500, x5=1500)), (N_SKEW_MIN, 1024, 150, _w(x0=1500, x7=500)), (N_MID[1], 256, -1, _w(x3=500, x4=1500)), (N_SKEW, 512, 400, _w(x7=1500, x1=500))]
)
TILE_CHUNKS = (1, 2, 4, 8, 16)  # GP_TUNE_TILE_CHUNKS: chunks per wave of a fixed tile
FIXED_BATCH = (5_000, 4_096, 4_097)
