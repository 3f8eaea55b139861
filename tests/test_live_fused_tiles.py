"""CPU: the tile sequence of the fused live launch (tests/helpers/live_fused_tiles.py): the order the kernel runs its tiles in gives the head
tiles the rule "256 entries while 256 are pending, then the remainder" gives, takes 256 entries with every head tile but a workgroup's last, and
never has 768 entries pending -- for every shape of live counts the GPU cases walk, and for random ones."""
import random

import pytest

from helpers import live_fused_tiles as T

CASES = {
    'one sample': [1],
    'nothing live': [0, 0, 0, 0, 0],
    'all live': [256] * 5,
    'all live, ragged end': [256, 256, 1],
    'remainder 1': [256, 1],
    'remainder 255': [255],
    'full on the second': [140, 140, 140, 140, 140],
    'full on the third': [100, 100, 100, 100, 100],
    'full on the last': [55, 55, 55, 55, 55],
    'never full': [10, 0, 3, 0, 7],
    'worst case for the list': [255, 256, 256, 0, 256],
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_named_sequences(name):
    c = CASES[name]
    heads, rem = T.head_tiles(c)
    kinds, takes, most = T.schedule(c)
    assert kinds.count('T') == len(c) and kinds.count('H') == heads == -(-sum(c) // 256)
    assert all(t == 256 for t in takes[:-1]) and (not takes or takes[-1] == (rem or 256))
    assert most < T.ENTRIES


def test_examples():
    assert T.head_tiles([256] * 5) == (5, 0) and T.head_tiles([256, 1]) == (2, 1) and T.head_tiles([255]) == (1, 255) and T.head_tiles([0, 0]) == (0, 0)
    assert T.schedule([256] * 3)[0] == list('TTHHTH')               # the first head tile comes a trunk tile AFTER the one that filled the list
    assert T.schedule([0, 0])[0] == list('TT') and T.schedule([1])[0] == list('TH')
    assert T.first_full([140] * 5) == 2 and T.first_full([100] * 5) == 3 and T.first_full([55] * 5) == 5 and T.first_full([10] * 5) == 0
    assert T.schedule([255, 256, 256, 0, 256])[2] == 767           # the list's bound is reached and not passed


def test_random_sequences():
    rng = random.Random(5)
    for _ in range(2000):
        c = [rng.choice([0, 1, 31, 100, 128, 200, 255, 256, rng.randrange(257)]) for _ in range(rng.randrange(1, 12))]
        heads, rem = T.head_tiles(c)
        kinds, takes, most = T.schedule(c)
        assert kinds.count('H') == heads and sum(takes) == sum(c) and most < T.ENTRIES
        assert all(t == 256 for t in takes[:-1])


def test_group_counts_and_workspace():
    live = [True] * 300 + [False] * 300 + [True] * 50               # tiles of 256, 44 + 0, 0 + 50 live samples
    assert T.group_counts(live, 2) == [[256, 50], [44]] and T.group_counts(live, 3) == [[256], [44], [50]]
    assert T.groups(1) == 1 and T.groups(256) == 1 and T.groups(257) == 2 and T.groups(1 << 30) == 256
    assert T.workspace_bytes(1) == 768 * 520 + 256 and T.workspace_bytes(256 * 33) == 33 * 768 * 520 + 512
