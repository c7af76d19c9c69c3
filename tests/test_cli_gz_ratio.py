"""FQD_GZ_DEVICE_RATIO=high: the resident runs deflate their `.gz` outputs with the search mode of the device coder.  Every
such run writes a `.gz` that gzip inflates to exactly the bytes the same command writes to a plain output, smaller than
without the switch, and readable again as an input (the device inflater)."""
import gzip
import random
import subprocess

import pytest

from test_cli import exe, fastq, random_reads, run  # noqa: F401  (exe is a fixture)

HIGH = {"FQD_GZ_DEVICE_RATIO": "high"}


def reads_text(seed, n=6000, mate=1):
    rnd = random.Random(seed)
    seqs = random_reads(rnd, n, 1500, 100, 150, alphabet=b"ACGT")
    qual = [bytes(rnd.choice(b"FFFFFFFF:,#") for _ in s) for s in seqs]       # what a search finds matches in and a run coder does not
    return fastq([(b"A00123:45:HXXXXXXX:%d:%d:%d:%d %d:N:0:ACGTACGT" % (1 + k % 4, 1101 + k // 500, 1000 + (k * 7919) % 30000, 1000 + (k * 104729) % 38000, mate), seqs[k])
                  for k in range(n)], qual)


def test_a_misspelt_value_ends_the_run_before_any_output(exe, tmp_path):
    src, out = tmp_path / "in.fq", tmp_path / "out.fq.gz"
    src.write_bytes(reads_text(1, 100))
    r = run(exe, "-i", src, "-o", out, "--fast", env={"FQD_GZ_DEVICE_RATIO": "bogus"})
    assert r.returncode == 1
    assert "FQD_GZ_DEVICE_RATIO" in r.stderr and "bogus" in r.stderr
    assert not out.exists()


MODES = {
    "fast_se": (False, ["--fast"]),
    "fast_pe": (True, ["--fast"]),
    "unordered": (True, ["--fast", "--unordered"]),
    "compare_seq_tight": (False, ["--compare-seq", "tight"]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_high_ratio_outputs(exe, tmp_path, mode):
    paired, flags = MODES[mode]
    ins = [tmp_path / "r1.fq", tmp_path / "r2.fq"][:2 if paired else 1]
    for k, f in enumerate(ins):
        f.write_bytes(reads_text(40 + k if not paired else 40, mate=k + 1))

    def go(outs, sources=ins, env=None):
        args = ["-i", sources[0], "-o", outs[0]] + (["-u", sources[1], "-p", outs[1]] if paired else [])
        r = run(exe, *args, *flags, env=env, cwd=tmp_path)
        assert r.returncode == 0, r.stderr
        return r.stdout

    plain = [tmp_path / f"plain{k}.fq" for k in range(len(ins))]
    high = [tmp_path / f"high{k}.fq.gz" for k in range(len(ins))]
    dflt = [tmp_path / f"default{k}.fq.gz" for k in range(len(ins))]
    said = go(plain)
    assert go(high, env=HIGH) == said
    assert go(dflt) == said
    for p, h, d in zip(plain, high, dflt):
        assert p.stat().st_size > 100_000
        assert subprocess.run(["gzip", "-t", str(h)]).returncode == 0
        assert gzip.open(h, "rb").read() == p.read_bytes()
        assert gzip.open(d, "rb").read() == p.read_bytes()
        assert h.stat().st_size < d.stat().st_size, (h.stat().st_size, d.stat().st_size)
    # the high-mode files as INPUT: inflated on the device, the same result as from the plain files
    again = [tmp_path / f"again{k}.fq" for k in range(len(ins))]
    from_plain = [tmp_path / f"from_plain{k}.fq" for k in range(len(ins))]
    assert go(again, sources=high) == go(from_plain, sources=plain)
    for a, b in zip(again, from_plain):
        assert a.read_bytes() == b.read_bytes()
