"""Seeded inputs of the PDHMM edge tests (tests/test_pdhmm_edges.py on the GPU, tests/test_pdhmm_edge_inputs_cpu.py for
what the inputs themselves must satisfy).  No GPU and no oracle in here: geometry and bytes only.

The kernels cut a read of R bases into n_blocks = (R + RPL) / RPL row blocks of RPL rows (row 0 of the matrices included,
the pad rows in front of it); up to 64 blocks are packed into one wavefront, more run as stripes of 64 blocks whose FIRST
stripe holds the remainder in its high lanes (pdhmm_kernel.h: pdhmm_fwd_kernel, PdJob::setup_at).  Every length below is
derived from RPL, and a CPU test compares RPL with GKL_PD_RPL of gkl_amd/csrc/pdhmm_job_layout.h."""
import numpy as np

from gkl_amd.pdhmm_batch import PdhmmBatch

RPL = 6                                   # rows per lane (GKL_PD_RPL)
LANES = 64
PACKED_MAX = LANES * RPL - 1              # 383: the longest read that is packed; one more base runs striped
ACGT = np.frombuffer(b"ACGT", dtype=np.int8)
SNP, DEL_START, DEL_END = 1, 2, 4


# ------------------------------------------------------------------ geometry, as PdJob::setup_at / pdhmm_fwd_kernel derive it
def n_blocks(R):
    return (R + RPL) // RPL


def n_stripes(R):
    return (n_blocks(R) + LANES - 1) // LANES


def first_cnt(R):
    """Blocks (= active lanes) of the first stripe."""
    return n_blocks(R) - LANES * (n_stripes(R) - 1)


def seam_rows(R):
    """Per seam between two stripes: (read index of the last row of the stripe above, of the first row of the stripe
    below).  Block b holds the rows b * RPL - pads .. + RPL - 1, where -1 is row 0 of the matrices (no read base: the index
    is then None) and the pads lie in front of it."""
    pads = n_blocks(R) * RPL - R
    out = []
    for st in range(n_stripes(R) - 1):
        last_block = first_cnt(R) + st * LANES - 1
        last = last_block * RPL - pads + RPL - 1
        assert -1 <= last and last + 1 < R
        out.append((last if last >= 0 else None, last + 1))
    return out


# ------------------------------------------------------------------ one pair whose likelihood stays far from underflow
def related_hap(rng, H, flag_rate=0.03):
    hap = ACGT[rng.randint(0, 4, H)].copy()
    pd = np.zeros(H, np.int8)
    j = 0
    while j < H:
        u = rng.random_sample()
        if u < flag_rate * 0.5:
            pd[j] = SNP | int(rng.randint(1, 16)) << 3            # SNP column, random allele set
        elif u < flag_rate * 0.85:
            span = int(rng.randint(1, 4))                           # DEL_START ... DEL_END over 1..3 columns
            if j + span < H:
                pd[j] |= DEL_START
                pd[j + span] |= DEL_END
                j += span
        elif u < flag_rate:
            pd[j] = int(rng.randint(0, 128))                        # an arbitrary flag byte
        j += 1
    return hap, pd


def related_read(rng, hap, R, sub_rate=0.02):
    """A slice of the haplotype when it is long enough, else the haplotype repeated to R bases; ~2 % substitutions.  Only
    A, C, G, T: every engine of the reference accepts such a read under a SNP column."""
    H = hap.size
    if R <= H:
        off = int(rng.randint(0, H - R + 1))
        read = hap[off:off + R].copy()
    else:
        read = np.tile(hap, R // H + 1)[:R].copy()
    flip = rng.random_sample(R) < sub_rate
    read[flip] = ACGT[rng.randint(0, 4, int(flip.sum()))]
    return read


def related_pair(rng, R, H, qual=(20, 40), indel=(30, 45), gcp=(8, 12), flag_rate=0.03, sub_rate=0.02):
    hap, pd = related_hap(rng, H, flag_rate)
    read = related_read(rng, hap, R, sub_rate)
    q = lambda lohi: rng.randint(lohi[0], lohi[1] + 1, R).astype(np.int8)  # noqa: E731
    return hap, pd, read, q(qual), q(indel), q(indel), q(gcp)


# ------------------------------------------------------------------ A: stripe geometry
STRIPE_R = [PACKED_MAX - 1, PACKED_MAX, PACKED_MAX + 1, PACKED_MAX + 2,               # 382 383 | 384 (first stripe: one lane, row 0 only) 385
            PACKED_MAX + RPL, PACKED_MAX + RPL + 1, PACKED_MAX + RPL + 2,             # 389 390 391: the first stripe gains its second lane
            2 * LANES * RPL - 2, 2 * LANES * RPL - 1, 2 * LANES * RPL, 2 * LANES * RPL + 1,   # 766 767 (64 full lanes) | 768 (three stripes) 769
            3 * LANES * RPL - 1, 3 * LANES * RPL, 3 * LANES * RPL + 1]                # 1151 | 1152 (four stripes: a carry buffer reused) 1153
STRIPE_COUNTS = [1, 1, 2, 2, 2, 2, 2, 2, 2, 3, 3, 3, 4, 4]
PAIRS_PER_R = 3


def stripe_pairs():
    rng = np.random.RandomState(6001)
    return [related_pair(rng, R, int(rng.randint(R, R + 41))) for R in STRIPE_R for _ in range(PAIRS_PER_R)]


def stripe_batch():
    return PdhmmBatch.from_pairs(stripe_pairs())


# ------------------------------------------------------------------ B: carry columns (flushed and read 64 at a time)
CARRY_R = [LANES * RPL, 2 * LANES * RPL, 3 * LANES * RPL + 1]                         # 384 768 1153
CARRY_H = [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 191, 192, 193]


def carry_pairs():
    """Hundreds of inserted bases per pair: gap continuation 1..2 keeps the sums far from underflow."""
    rng = np.random.RandomState(6002)
    return [related_pair(rng, R, H, gcp=(1, 2)) for R in CARRY_R for H in CARRY_H]


def carry_batch():
    return PdhmmBatch.from_pairs(carry_pairs())


# ------------------------------------------------------------------ C: packed geometry
PACKED_R = [1, RPL - 1, RPL, RPL + 1, 2 * RPL - 1, 2 * RPL, 2 * RPL + 1,             # 1 5 6 7 11 12 13
            PACKED_MAX - RPL, PACKED_MAX - RPL + 1, PACKED_MAX - RPL + 2, PACKED_MAX]   # 377 378 379 383
PACKED_H = [1, 2, 3, 4, 5, 6, 7, 63, 64, 65]


def packed_sides():
    """(reads, haplotypes): reads[k] is related to haplotype k % len(PACKED_H)."""
    rng = np.random.RandomState(6003)
    haps = [related_hap(rng, H, flag_rate=0.1) for H in PACKED_H]
    reads = []
    for R in PACKED_R:
        for k, (hap, _) in enumerate(haps):
            q = lambda lo, hi: rng.randint(lo, hi + 1, R).astype(np.int8)  # noqa: E731
            reads.append((related_read(rng, hap, R), q(20, 40), q(30, 45), q(30, 45), q(8, 12)))
    return reads, haps


def packed_batch():
    """All len(PACKED_R) * len(PACKED_H) pairs in one batch: every read length against every haplotype length."""
    reads, haps = packed_sides()
    return PdhmmBatch.from_pairs([(*haps[k % len(haps)], *r) for k, r in enumerate(reads)])


def sides_as_batches(reads, haps):
    """The two sides as compute_cross takes them."""
    one = np.zeros(1, np.int8)
    return (PdhmmBatch.from_pairs([(one, one, *r) for r in reads]),
            PdhmmBatch.from_pairs([(hb, hp, one, one, one, one, one) for hb, hp in haps]))


def cross_pairs(reads, haps):
    """reads x haplotypes, read-major, as one paired batch."""
    return PdhmmBatch.from_pairs([(hb, hp, *r) for r in reads for hb, hp in haps])


# ------------------------------------------------------------------ D: every quality byte
QUAL_H = 420
QUAL_R = [128, 400]                       # packed, striped
HAP_KINDS = ["table", "many-classes", "odd-base"]


def kind_haps(seed=6004, H=QUAL_H):
    """Three haplotypes over ONE random base string, so that a read related to it is related to all three: at most six column
    classes (table kernel), seven or more (predicate kernel), a base outside ACGTN (byte-comparing kernel) -- the kinds
    test_pdhmm_gpu_table_kernel_routing_and_parity builds."""
    rng = np.random.RandomState(seed)
    base = ACGT[rng.randint(0, 4, H)].copy()
    out = []
    for kind in HAP_KINDS:
        hb, pd = base.copy(), np.zeros(H, np.int8)
        n_snp = {"table": 1, "many-classes": 4, "odd-base": 1}[kind]
        cols = rng.choice(np.arange(8, H - 8), 2 * n_snp + 1, replace=False)
        for k in range(n_snp):                                      # SNP kind k: base k, its own allele set, on two columns
            for j in cols[2 * k:2 * k + 2]:
                hb[j] = ACGT[k]
                pd[j] = SNP | [3, 5, 9, 6][k] << 3
        if kind == "odd-base":
            hb[cols[-1]] = ord("r")
        j = int(rng.randint(20, H - 40))
        pd[j] |= DEL_START
        pd[j + 2] |= DEL_END
        out.append((hb, pd))
    return base, out


def quality_reads(base, R, seed):
    """Reads of R bases related to `base` in which row i carries byte i of ONE of the four quality arrays (the others stay in
    their plain ranges): name -> (bases, qual, ins, del, gcp)."""
    rng = np.random.RandomState(seed)
    i = np.arange(R)
    plain = lambda lo, hi: rng.randint(lo, hi + 1, R).astype(np.int8)  # noqa: E731
    mk = lambda **kw: (related_read(rng, base, R), kw.get("qual", plain(20, 40)), kw.get("ins", plain(30, 45)),  # noqa: E731
                       kw.get("dele", plain(30, 45)), kw.get("gcp", plain(8, 12)))
    reads = {}
    if R <= 128:
        reads["qual 0..127"] = mk(qual=(i % 128).astype(np.int8))
        reads["qual -128..-1"] = mk(qual=(i % 128 - 128).astype(np.int8))
    else:
        reads["qual all 256"] = mk(qual=(i % 256).astype(np.uint8).view(np.int8))
    reads["ins = del"] = mk(ins=(i % 128).astype(np.int8), dele=(i % 128).astype(np.int8))                 # the diagonal, (0,0), (127,127)
    reads["ins up, del down"] = mk(ins=(i % 128).astype(np.int8), dele=(127 - i % 128).astype(np.int8))    # (0,127) and (127,0)
    # gap continuation 0 makes 1 - egc exactly 0: in the FIRST row nothing could leave row 0 and the sum would be 0, so
    # byte 0 sits at row 64 (and 192, 320 of the long read), where the match matrix carries the pair on
    reads["gcp 0..127"] = mk(gcp=((i + 64) % 128).astype(np.int8))
    return reads


def quality_sides():
    """(names, reads, haplotypes)."""
    base, haps = kind_haps()
    names, reads = [], []
    for R in QUAL_R:
        for name, r in quality_reads(base, R, 6100 + R).items():
            names.append(f"{name}, {R} bases")
            reads.append(r)
    return names, reads, haps


def quality_batch():
    _, reads, haps = quality_sides()
    return cross_pairs(reads, haps)


def holds_byte_255(b):
    """Per pair: does a base quality of its read hold byte -1?  The kernels and the oracle give index 255 entry 0 of the
    255-entry error table; every engine of the reference reads one entry past its table there (docs/NOTES.md), so such a
    pair has no reference value and stays out of the scalar tail of the default-mode tests."""
    q = b.read_qual.reshape(b.batch, b.max_read_len)
    return np.array([bool((q[k, :b.read_lengths[k]] == -1).any()) for k in range(b.batch)])


def without_byte_255(b):
    """The batch with base-quality byte -1 replaced by -2 (index 254, the table's last entry)."""
    keep = b.subset(np.arange(b.batch))
    q = keep.read_qual.reshape(b.batch, b.max_read_len).copy()
    for k in range(b.batch):
        row = q[k, :b.read_lengths[k]]
        row[row == -1] = -2
    keep.read_qual = q.reshape(-1)
    return keep


# ------------------------------------------------------------------ E: underflow ladders
LADDER_H = 40
LADDERS = {"packed": dict(gcp=20, R=list(range(296, 324))),
           "striped": dict(gcp=15, R=list(range(LANES * RPL, LANES * RPL + 55, 2)))}        # 384, 386 .. 438
# log10 of a sum that is subnormal once scaled by 2^1020: below the smallest normal, at or above the smallest subnormal
SUBNORMAL_WINDOW = (float(np.log10(5e-324) - 1020 * np.log10(2.0)) - 0.01, float(np.log10(2.2250738585072014e-308) - 1020 * np.log10(2.0)))


def ladder_batch(which):
    """A haplotype of C against reads of A, every quality 40: each further base costs one more gap-continuation factor, and the
    sum walks down through the normal range, the subnormals and out of fp64."""
    spec = LADDERS[which]
    hap, pd = np.full(LADDER_H, ord("C"), np.int8), np.zeros(LADDER_H, np.int8)
    pairs = []
    for R in spec["R"]:
        q40 = np.full(R, 40, np.int8)
        pairs.append((hap, pd, np.full(R, ord("A"), np.int8), q40, q40, q40, np.full(R, spec["gcp"], np.int8)))
    return PdhmmBatch.from_pairs(pairs)
