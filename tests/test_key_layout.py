"""tests/key_layout.py against itself: the batch (numpy) forms equal the scalar statements, a pair's words and the
padded key are laid out as documented, and hash_end never returns kSkipHash.  No GPU, no native code."""
import random

import numpy as np

import key_layout as kl


def test_batch_forms_equal_the_scalar_statements():
    rnd = random.Random(7)
    for L in (1, 17, 31, 32, 33, 63, 64, 65, 100, 128, 149, 150, 151, 250, 256, 384, 450):
        rows = np.array([[rnd.choice(b"ACGTN") for _ in range(L)] for _ in range(6)], np.uint8)
        rows[0, :] = ord("N"); rows[1, :] = ord("G"); rows[2, :] = ord("A")
        W = kl.words_of_rows(rows)
        assert W.shape == (6, kl.seg_words(L))
        for i in range(6):
            assert [int(x) for x in W[i]] == kl.expected_words(bytes(rows[i])), (L, i)
        H = kl.hashes_of_rows(L, W)
        L2 = max(1, L // 2 + 1)
        W2 = kl.words_of_rows(rows[:, :L2])
        H2 = kl.hashes_of_rows(L, W, L2, W2)
        for i in range(6):
            w, w2 = [int(x) for x in W[i]], [int(x) for x in W2[i]]
            assert int(H[i]) == kl.expected_hash(L, 0, w), (L, i)
            assert int(H2[i]) == kl.expected_hash(L, L2, w, w2), (L, i)


def test_pair_and_padded_layouts():
    a, b = b"ACGTN" * 30, b"GGN" * 11
    assert kl.expected_pair_words(a, b) == kl.expected_words(a) + kl.expected_words(b)
    assert len(kl.expected_pair_words(a, b)) == kl.seg_words(150) + kl.seg_words(33)
    p = kl.expected_padded(a, b, 160, 130)
    assert len(p) == kl.padded_key_words(160, 130) == 1 + 8 + 8
    assert p[0] == 150 | (33 << 32) and p[1:9] == kl.expected_words(a) and p[9:12] == kl.expected_words(b) and p[12:] == [0] * 5
    s = kl.expected_padded(b"ACG", None, 64)
    assert s == [3, kl.expected_words(b"ACG")[0], 0, 0]
    # the two hashes of a padded key differ in what they run over: the read (source) / all K words (owner)
    assert kl.expected_opaque_hash(s) == kl.hash_end(kl.hash_chain(4, s))
    assert kl.expected_hash(3, 0, s[1:3]) != kl.expected_opaque_hash(s)


def _unmix(h):
    """Inverse of the two xor-shift-multiply rounds of hash_end (before its clamp)."""
    inv1, inv2 = pow(0xFF51AFD7ED558CCD, -1, 1 << 64), pow(0xC4CEB9FE1A85EC53, -1, 1 << 64)
    unshift = lambda x: x ^ (x >> 33)                      # x ^= x >> 33 is its own inverse for shifts >= 32
    h = unshift(h)
    h = (h * inv2) & kl.M64
    h = unshift(h)
    h = (h * inv1) & kl.M64
    return unshift(h)


def test_hash_end_never_returns_the_skip_value():
    x = _unmix(kl.SKIP_HASH)                                # the one chain state that would mix to all ones
    assert kl.hash_end(x) == kl.SKIP_HASH - 1
    assert kl.hash_end(_unmix(kl.SKIP_HASH - 1)) == kl.SKIP_HASH - 1
    assert kl.hash_end(_unmix(12345)) == 12345
    got = kl._hash_end_rows(np.array([x, _unmix(12345)], np.uint64))
    assert [int(v) for v in got] == [kl.SKIP_HASH - 1, 12345]
    assert kl.weak(kl.M64) == 0xFFFFFFC0
