"""The tile sequence of a workgroup of nerf_mlp_i8s_fused_kernel (csrc/mlp_i8f.hip), restated: trunk tiles in their static order, head tiles of
256 entries while 256 are pending, then one more for the remainder.

`head_tiles` is the rule itself.  `schedule` is the order the kernel runs them in: the kind of the NEXT tile is fixed at the top of the tile in
hand, from what is pending there less what a head tile is about to take (the weight ring copies the next tile's first blocks under this tile's
last ones), so a head tile may come one trunk tile later than the rule read naively says -- the number of head tiles is the same, and the
list never holds 768 entries."""
TILE = 256
ENTRIES = 768                          # a workgroup's list (kFusedEntries)
MAX_GROUPS = 256                       # lists a workspace holds at most (kFusedMaxGroups)
LIST_BYTES = ENTRIES * 520


def head_tiles(live_counts):
    """-> (head tiles, entries of the last one if it is a remainder else 0) of a workgroup whose trunk tiles list live_counts samples"""
    pending, heads = 0, 0
    for c in live_counts:
        pending += c
        while pending >= TILE:
            pending -= TILE
            heads += 1
    return heads + (1 if pending else 0), pending


def schedule(live_counts):
    """-> (kinds 'T' / 'H' in the order run, entries taken by each head tile, the largest number of entries pending) as the kernel decides them"""
    kinds, takes, most = [], [], 0
    appended = consumed = done = 0
    head = False
    while True:
        pending = appended - consumed
        if head and pending == 0:
            break
        take = min(pending, TILE) if head else 0
        more = (done if head else done + 1) < len(live_counts)
        next_head = pending - take >= TILE or not more
        if head:
            consumed += take
            takes.append(take)
        else:
            assert pending < 2 * TILE
            appended += live_counts[done]
            done += 1
        most = max(most, appended - consumed)
        kinds.append('H' if head else 'T')
        head = next_head
    assert done == len(live_counts) and appended == consumed
    return kinds, takes, most


def first_full(live_counts):
    """the trunk tile (1-based) after which 256 entries are pending for the first time, 0 if never"""
    pending = 0
    for k, c in enumerate(live_counts):
        pending += c
        if pending >= TILE:
            return k + 1
        # (head tiles only run from 256 up: nothing is taken before)
    return 0


def groups(n):
    return min((n + TILE - 1) // TILE, MAX_GROUPS)


def workspace_bytes(n):
    """nm_mlp_live_fused_workspace_bytes: a list per workgroup, then two int32 per workgroup rounded up to 256 bytes"""
    return groups(n) * LIST_BYTES + (groups(n) * 8 + 255) // 256 * 256


def group_counts(live, grid):
    """live: flat bools, one per sample -> per workgroup the live samples of each of its trunk tiles (tile t belongs to workgroup t % grid)"""
    n = len(live)
    ntiles = (n + TILE - 1) // TILE
    per_tile = [int(sum(live[t * TILE:(t + 1) * TILE])) for t in range(ntiles)]
    return [per_tile[wg::grid] for wg in range(grid)]
