"""GPU checks of the sequence-based primitives (fqd_sort_seqs, fqd_seq_heads: csrc/fqd_seq.hip).

- fqd_sort_seqs gives the permutation of fqd_sort_tags — an independent sorter of the same order (FastqView::cmp) —
  on spans that include the '\\n', for ragged reads and for 20 M x 150 bp synthetic reads
- fqd_seq_heads equals the reference's scan (tests/seq_reference.py) on adversarial lists, including one 2 M-record
  tail-hamming segment without a certain cut
- reads with more than 32768 key bits of varying bytes (no key-width cap), and the refusal of a NUL byte."""
import numpy as np
import pytest
import torch

from fastq_dupaway_amd import Engine
from fastq_dupaway_amd._lib import FqdError, SEQ_HAMMING, SEQ_LOOSE, SEQ_TIGHT
import seq_reference as ref

pytestmark = pytest.mark.gpu
MODE = {ref.TIGHT: SEQ_TIGHT, ref.LOOSE: SEQ_LOOSE, ref.HAMMING: SEQ_HAMMING}


def dev(a):
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host_u32(t, n):
    return t.cpu().numpy().view(np.uint32)[:n]


def spans(seqs):
    """One byte array holding seq + '\\n' per record; (data, offsets, lengths without the '\\n')."""
    lens = np.array([len(s) for s in seqs], dtype=np.uint32)
    offs = np.zeros(len(seqs), np.uint64)
    if len(seqs) > 1:
        offs[1:] = np.cumsum(lens[:-1].astype(np.uint64) + 1)
    data = np.frombuffer(b"".join(s + b"\n" for s in seqs) + b"\0" * 16, dtype=np.uint8).copy()
    return data, offs, lens


def device_order(e, mates):
    """perm and heads of every mode for a list of records (tuples of 1 or 2 mates)."""
    n = len(mates)
    ds = [tuple(dev(x) for x in spans([m[k] for m in mates])) for k in range(len(mates[0]))]
    t = [(d, o, l, n) for d, o, l in ds]
    perm = torch.empty(n, dtype=torch.int32, device="cuda")
    e.sort_seqs(t[0], perm, t[1] if len(t) > 1 else None)
    return t, perm


def test_sort_seqs_equals_sort_tags_ragged():
    rng = np.random.default_rng(1)
    n = 1_000_000
    lens = rng.integers(0, 201, n).astype(np.uint32)
    lens[rng.random(n) < 0.05] = 0
    alpha = np.frombuffer(b"ACGTNacgtRYK", np.uint8)
    total = int(lens.sum()) + n
    data = rng.choice(alpha[:5], size=total + 16, p=[.24, .24, .24, .24, .04]).astype(np.uint8)
    data[rng.random(total + 16) < 0.01] = alpha[7]
    offs = np.zeros(n, np.uint64)
    offs[1:] = np.cumsum(lens[:-1].astype(np.uint64) + 1)
    data[(offs + lens).astype(np.int64)] = ord("\n")
    dup = rng.random(n) < 0.3                                # exact duplicates and prefixes of earlier records
    src = rng.integers(0, n, n)
    offs[dup] = offs[src[dup]]
    cut = dup & (rng.random(n) < 0.5)
    lens[dup] = np.where(cut[dup], np.minimum(lens[src[dup]], rng.integers(0, 201, int(dup.sum()))), lens[src[dup]])
    # a copied record shares its source's bytes; a cut copy is a prefix of them (no '\n' right behind it)
    d = dev(data)
    o, l = dev(offs), dev(lens)
    perm = torch.empty(n, dtype=torch.int32, device="cuda")
    perm_t = torch.empty(n, dtype=torch.int32, device="cuda")
    with Engine(segments=1) as e:
        e.sort_seqs((d, o, l, n), perm)
    # every record: the host's stable sort by bytes + '\n'
    hb = data.tobytes()
    keys = [hb[int(offs[i]):int(offs[i]) + int(lens[i])] + b"\n" for i in range(n)]
    exp = np.array(sorted(range(n), key=keys.__getitem__), dtype=np.uint32)
    assert np.array_equal(host_u32(perm, n), exp)
    # and fqd_sort_tags agrees where every span carries its own '\n' (records that are not cut copies)
    keep = ~cut
    idx = np.nonzero(keep)[0]
    m = len(idx)
    t_off, t_len = offs[idx], lens[idx]
    with Engine(segments=1) as e:
        e.sort_seqs((d, dev(t_off), dev(t_len), m), perm)
        e.sort_tags(d, dev(t_off), dev(t_len + 1), m, perm_t)
    assert np.array_equal(host_u32(perm, m), host_u32(perm_t, m))


def test_sort_seqs_equals_sort_tags_20m_x_150():
    n, L = 20_000_000, 150
    bases = torch.empty(n * L + 64, dtype=torch.uint8, device="cuda")
    with Engine(segments=1) as e:
        e.synth_reads(7, 0, n, L, 300, 0, bases)
        offs = torch.arange(n, dtype=torch.int64, device="cuda") * L
        lens = torch.full((n,), L, dtype=torch.int32, device="cuda")
        perm = torch.empty(n, dtype=torch.int32, device="cuda")
        perm_t = torch.empty(n, dtype=torch.int32, device="cuda")
        e.sort_seqs((bases, offs, lens, n), perm)
        e.sort_tags(bases, offs, lens, n, perm_t)            # equal lengths: the '\n' changes nothing
        assert torch.equal(perm, perm_t)


def adversarial_lists(rng):
    base = b"ACGTACGGTCAGTTAGCAGGATCCAGTAGCAT" * 3
    out = []
    out.append([(base[:rng.integers(0, len(base) + 1)],) for _ in range(3000)])                     # prefix chains, empty reads
    out.append([(b"",)] * 5 + [(b"A",), (b"",), (b"AC",)])
    mut = []
    for _ in range(3000):
        s = bytearray(base)
        for _ in range(rng.integers(0, 3)):
            s[rng.integers(0, len(s))] = b"ACGT"[rng.integers(0, 4)]
        mut.append((bytes(s),))
    out.append(mut)                                                                                # hamming chains
    pairs = []
    for _ in range(3000):
        c1, c2 = int(rng.integers(0, 30)), int(rng.integers(0, 30))
        pairs.append((base[:c1], base[:c2] if rng.random() < 0.5 else base[:30 - c1]))              # opposite-sided overlaps
    out.append(pairs)
    pairs2 = [(mut[i][0], mut[(i * 7) % len(mut)][0][:60]) for i in range(len(mut))]
    out.append(pairs2)
    return out


@pytest.mark.parametrize("mode,d", [(ref.TIGHT, 2), (ref.LOOSE, 2), (ref.HAMMING, 0), (ref.HAMMING, 1), (ref.HAMMING, 3)])
def test_heads_match_restatement(mode, d):
    rng = np.random.default_rng(10 + mode * 7 + d)
    with Engine(segments=2) as e:
        for mates in adversarial_lists(rng):
            n = len(mates)
            t, perm = device_order(e, mates)
            p = host_u32(perm, n)
            assert list(p) == ref.sorted_order(mates)
            head = torch.empty(n, dtype=torch.uint8, device="cuda")
            got = e.seq_heads(t[0], perm, MODE[mode], d, head, t[1] if len(t) > 1 else None)
            exp = ref.heads(mode, d, [mates[i] for i in p])
            assert head.cpu().numpy().tolist() == exp
            assert got == sum(exp)


def test_hamming_segment_of_2m_without_certain_cut():
    # every record = base with at most one substitution, so neighbours differ in at most 2 = 2d places (d = 1): no
    # certain head anywhere, the whole sorted list is one segment walked by one wave
    n, L, d = 2_000_000, 150, 1
    rng = np.random.default_rng(3)
    base = rng.choice(np.frombuffer(b"ACGT", np.uint8), L).astype(np.uint8)
    pos = rng.integers(0, L, n)
    ch = rng.choice(np.frombuffer(b"ACGT", np.uint8), n).astype(np.uint8)
    data = np.tile(base, n)
    data[np.arange(n) * L + pos] = ch
    offs = (np.arange(n, dtype=np.uint64) * L).astype(np.uint64)
    lens = np.full(n, L, np.uint32)
    d_data, d_off, d_len = dev(np.concatenate([data, np.zeros(16, np.uint8)])), dev(offs), dev(lens)
    perm = torch.empty(n, dtype=torch.int32, device="cuda")
    head = torch.empty(n, dtype=torch.uint8, device="cuda")
    with Engine(segments=1) as e:
        e.sort_seqs((d_data, d_off, d_len, n), perm)
        got = e.seq_heads((d_data, d_off, d_len, n), perm, SEQ_HAMMING, d, head)
    p = host_u32(perm, n)
    # the scan, on the (position, byte) of each record's substitution (none when the byte is the base's)
    eff_p = np.where(ch != base[pos], pos, -1)[p]
    eff_c = ch[p]
    exp = np.zeros(n, np.uint8)
    hp, hc = None, None
    for k in range(n):
        xp, xc = int(eff_p[k]), int(eff_c[k])
        if hp is None:
            dist = 99
        elif hp == xp:
            dist = 0 if (xp < 0 or hc == xc) else 1
        else:
            dist = (hp >= 0) + (xp >= 0)
        if dist > d:
            exp[k] = 1; hp, hc = xp, xc
    assert np.array_equal(head.cpu().numpy(), exp)
    assert got == int(exp.sum())
    # the restatement itself on a prefix
    seqs = [(data[int(i) * L:(int(i) + 1) * L].tobytes(),) for i in p[:3000]]
    assert ref.heads(ref.HAMMING, d, seqs) == exp[:3000].tolist()


def test_long_reads_no_key_width_cap():
    # reads of 12000 varying bytes: 12000 x 4 bits > 32768 key bits (fqd_sort_tags refuses such keys)
    rng = np.random.default_rng(4)
    alpha = np.frombuffer(b"ACGTNacgtRYKMSWB", np.uint8)
    shared = rng.choice(alpha, 11990).tobytes()
    seqs = [shared + rng.choice(alpha, int(rng.integers(0, 10))).tobytes() for _ in range(300)]
    seqs += [rng.choice(alpha, 12000).tobytes() for _ in range(50)]
    seqs += [seqs[5], seqs[5][:6000], seqs[301]]
    mates = [(s,) for s in seqs]
    with Engine(segments=1) as e:
        t, perm = device_order(e, mates)
        assert list(host_u32(perm, len(mates))) == ref.sorted_order(mates)
        for mode in (ref.TIGHT, ref.LOOSE, ref.HAMMING):
            head = torch.empty(len(mates), dtype=torch.uint8, device="cuda")
            e.seq_heads(t[0], perm, MODE[mode], 2, head)
            p = host_u32(perm, len(mates))
            assert head.cpu().numpy().tolist() == ref.heads(mode, 2, [mates[i] for i in p])


def test_nul_byte_is_refused():
    mates = [(b"ACGT",), (b"AC\x00T",), (b"A",)]
    with Engine(segments=1) as e:
        with pytest.raises(FqdError, match="below"):
            device_order(e, mates)
