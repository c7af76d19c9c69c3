"""The key format and the placement hash, stated in plain Python — independent of csrc/fqd_device.hpp.

What the device's encoders have to write for a read, word for word, and the 64 bits they have to hash it to:
  * expected_words(seq)               one mate's key words
  * expected_pair_words(s1, s2)       a pair's: mate 1's words, then mate 2's
  * expected_padded(...)              the padded key of fqd_encode_padded
  * expected_hash(len0, len1, w0, w1) the hash every encoder, hash_keys_kernel and rehash_kernel must agree on
  * expected_opaque_hash(words)       the hash of an opaque (padded) key on its owner
CPU only; tests/test_packer_host.py checks it against the host compile of the packer, the GPU tests
(test_gpu_key_words.py) hold the device's output against it.
"""
CODE = {ord("A"): 0, ord("C"): 1, ord("T"): 2, ord("G"): 3, ord("N"): 3}

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1


def expected_words(seq: bytes):
    """Independent statement of the layout in fqd_device.hpp: per 64-base block
    [codes group 0][codes group 1 if any][N mask]; inside a 32-base group, base
    4k+j (dword k, byte j) -> codes bits 32*(k//4) + 8j + 2(k%4), mask bit 8j + k."""
    words = []
    for blk in range(0, len(seq), 64):
        part = seq[blk:blk + 64]
        mask = 0
        for gi, g in enumerate(range(0, len(part), 32)):
            w = 0
            for b, c in enumerate(part[g:g + 32]):
                k, j = divmod(b, 4)
                w |= CODE[c] << (32 * (k // 4) + 8 * j + 2 * (k % 4))
                if c == ord("N"):
                    mask |= 1 << (32 * gi + 8 * j + k)
            words.append(w)
        words.append(mask)
    return words


def seg_words(length: int) -> int:
    """Key words of one mate: a codes word per 32 bases and a mask word per 64."""
    return (length + 31) // 32 + (length + 63) // 64


def expected_pair_words(seq1: bytes, seq2: bytes):
    """A pair's key: mate 1's words, then mate 2's (each mate packed on its own)."""
    return expected_words(seq1) + expected_words(seq2)


def padded_key_words(max_len0: int, max_len1: int = 0) -> int:
    """fqd_padded_key_words: the header word and room for the longest read of each mate."""
    return 1 + seg_words(max_len0) + seg_words(max_len1)


def expected_padded(seq1: bytes, seq2, max_len0: int, max_len1: int = 0):
    """The padded key of fqd_encode_padded (without the hash word in front of it):
    [len0 | len1 << 32][mate 1's words][mate 2's words][zeros up to padded_key_words(max_len0, max_len1)]."""
    len1 = len(seq2) if seq2 is not None else 0
    words = [len(seq1) | (len1 << 32)] + expected_words(seq1) + (expected_words(seq2) if seq2 is not None else [])
    K = padded_key_words(max_len0, max_len1)
    assert len(words) <= K
    return words + [0] * (K - len(words))


# ---- the placement hash: 64-bit wrap-around arithmetic -----------------------------------------------
HASH_SEED = 0x9E3779B97F4A7C15
HASH_MUL = 0x9FB21C651E98DF25
SKIP_HASH = M64                          # "no record here" in a batch's hash array: no record's own hash takes it


def hash_begin(len0: int, len1: int = 0) -> int:
    h = HASH_SEED ^ (len0 | (len1 << 32))
    h = (h * HASH_MUL) & M64
    return h ^ (h >> 32)


def hash_word(h: int, w: int) -> int:
    """One key word into the chain: two Feistel halves over the 32-bit halves of h ^ w."""
    x = h ^ w
    lo, hi = x & M32, x >> 32
    hi ^= ((lo & 0xFFFFFF) * 0x9E3779) & M32
    lo = (lo + (((hi << 15) | (hi >> 17)) & M32)) & M32
    return (hi << 32) | lo


def hash_end(h: int) -> int:
    h ^= h >> 33
    h = (h * 0xFF51AFD7ED558CCD) & M64
    h ^= h >> 33
    h = (h * 0xC4CEB9FE1A85EC53) & M64
    h ^= h >> 33
    return SKIP_HASH - 1 if h == SKIP_HASH else h          # the clamp: kSkipHash is never a record's hash


def hash_chain(length: int, words) -> int:
    h = hash_begin(length, 0)
    for w in words:
        h = hash_word(h, w)
    return h


def expected_hash(len0: int, len1: int, words0, words1=None) -> int:
    """Each mate is chained on its own from hash_begin(len, 0).  Single-end (words1 is None): hash_end(chain0).
    Paired: hash_pair(chain0, chain1) = hash_end(hash_word(chain0, chain1))."""
    c0 = hash_chain(len0, words0)
    if words1 is None:
        return hash_end(c0)
    return hash_end(hash_word(c0, hash_chain(len1, words1)))


def expected_opaque_hash(words) -> int:
    """Opaque keys (FQD_OPAQUE_KEYS: the padded keys on their owner, header word first) are K words of which nothing
    is known: hash_keys_kernel / rehash_kernel run ONE chain over all K of them from hash_begin(K, 0).  (The hash word
    fqd_encode_padded writes in front of a padded key is the read's own: expected_hash over its mates' words.)
    Read off the two kernels, NOT held against their output: no entry point hands out the hashes they write."""
    return hash_end(hash_chain(len(words), words))


def weak(h: int) -> int:
    """What FQD_FLAG_WEAK_HASH leaves of a hash: no tag, start slots that are multiples of 64."""
    return h & 0x00000000FFFFFFC0


# ---- the same two statements over whole batches (numpy; tests/test_key_layout.py holds them against the scalar forms) ----
def words_of_rows(rows):
    """expected_words of every row of an (n, L) uint8 array, as an (n, seg_words(L)) uint64 array."""
    import numpy as np
    n, L = rows.shape
    out = np.zeros((n, seg_words(L)), np.uint64)
    lut = np.zeros(256, np.uint64)
    for c, v in CODE.items():
        lut[c] = v
    code = lut[rows]
    is_n = (rows == ord("N")).astype(np.uint64)
    for p in range(L):
        blk, r = divmod(p, 64)
        gi, b = divmod(r, 32)
        k, j = divmod(b, 4)
        groups = 2 if L - 64 * blk > 32 else 1               # a block is [codes] x groups, then its mask word
        out[:, 3 * blk + gi] |= code[:, p] << np.uint64(32 * (k // 4) + 8 * j + 2 * (k % 4))
        out[:, 3 * blk + groups] |= is_n[:, p] << np.uint64(32 * gi + 8 * j + k)
    return out


def _hash_word_rows(h, w):
    import numpy as np
    x = h ^ w
    lo, hi = x & np.uint64(M32), x >> np.uint64(32)
    hi = hi ^ (((lo & np.uint64(0xFFFFFF)) * np.uint64(0x9E3779)) & np.uint64(M32))
    lo = (lo + (((hi << np.uint64(15)) | (hi >> np.uint64(17))) & np.uint64(M32))) & np.uint64(M32)
    return (hi << np.uint64(32)) | lo


def _hash_end_rows(h):
    import numpy as np
    with np.errstate(over="ignore"):
        h = h ^ (h >> np.uint64(33))
        h = h * np.uint64(0xFF51AFD7ED558CCD)
        h = h ^ (h >> np.uint64(33))
        h = h * np.uint64(0xC4CEB9FE1A85EC53)
        h = h ^ (h >> np.uint64(33))
    return np.where(h == np.uint64(SKIP_HASH), np.uint64(SKIP_HASH - 1), h)


def hashes_of_rows(len0, words0, len1=None, words1=None):
    """expected_hash of every row: words0 (n, seg_words(len0)) uint64, and for pairs words1 (n, seg_words(len1))."""
    import numpy as np

    def chain(length, words):
        h = np.full(words.shape[0], hash_begin(length, 0), np.uint64)
        for k in range(words.shape[1]):
            h = _hash_word_rows(h, words[:, k])
        return h
    c0 = chain(len0, words0)
    if words1 is None:
        return _hash_end_rows(c0)
    return _hash_end_rows(_hash_word_rows(c0, chain(len1, words1)))
