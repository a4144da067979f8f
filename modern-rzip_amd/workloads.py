"""Seeded synthetic workloads of SURVEY.md section 8d (no downloads: enwik8 is
not available offline).  Host generators return bytes; *_device build the large
BASELINE configurations directly in HBM with torch (plumbing only)."""
import numpy as np


def zipf_text(nbytes, seed=7, vocab=5000):
    """S1-style text: Zipf(1/rank) words from a seeded vocabulary, space
    separated, a newline every 20000 words."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(2, 11, size=vocab)
    words = [bytes(rng.integers(97, 123, size=int(k), dtype=np.uint8)) for k in lens]
    w = 1.0 / np.arange(1, vocab + 1)
    w /= w.sum()
    out = bytearray()
    while len(out) < nbytes:
        idx = rng.choice(vocab, size=20000, p=w)
        for i in idx:
            out += words[i]
            out += b" "
        out[-1:] = b"\n"
    return bytes(out[:nbytes])


def rep64k(nperiods, seed=1234, period=65536, first_period=0):
    """S2 "rep64k": a `period`-byte text block repeated; in period i the byte at
    (37*i) % period is replaced by i & 0xff."""
    base = np.frombuffer(zipf_text(period, seed=seed), dtype=np.uint8)
    arr = np.tile(base, nperiods).reshape(nperiods, period).copy()
    i = np.arange(first_period, first_period + nperiods)
    arr[np.arange(nperiods), (37 * i) % period] = (i & 0xFF).astype(np.uint8)
    return arr.tobytes()


def rep64k_device(nperiods, device, seed=1234, period=65536):
    """The same stream built in HBM: returns a uint8 torch tensor of nperiods*period bytes."""
    import torch
    base = torch.frombuffer(bytearray(zipf_text(period, seed=seed)), dtype=torch.uint8).to(device)
    out = base.repeat(nperiods).view(nperiods, period)
    i = torch.arange(nperiods, device=device, dtype=torch.int64)
    out[i, (37 * i) % period] = (i & 0xFF).to(torch.uint8)
    return out.view(-1)


def noise(nbytes, seed=99):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=nbytes, dtype=np.uint8).tobytes()


def tar_like(nbytes, seed=5):
    """S3-style mix: text members, noise members and exact duplicates of earlier
    members, 512-byte aligned."""
    rng = np.random.default_rng(seed)
    out = bytearray()
    members = []
    while len(out) < nbytes:
        kind = rng.random()
        size = int(2 ** rng.uniform(10, 17))
        if kind < 0.6 or not members:
            mem = zipf_text(size, seed=int(rng.integers(1, 1 << 30)))
        elif kind < 0.85:
            mem = noise(size, seed=int(rng.integers(1, 1 << 30)))
        else:
            mem = members[int(rng.integers(0, len(members)))]
        members.append(mem)
        out += mem
        out += bytes((-len(out)) % 512)
    return bytes(out[:nbytes])


def tar_like_fast(nbytes, seed=5, pool_bytes=48 << 20):
    """The S3 mix at sizes of a GiB and more without generating a GiB of Zipf text word by word: text members are
    slices of one text pool at random offsets (so parts of members repeat each other at distances of up to the whole
    stream), noise members come straight from the generator, 15 % are exact duplicates of earlier members;
    512-byte aligned like tar_like."""
    rng = np.random.default_rng(seed)
    pool = np.frombuffer(zipf_text(pool_bytes, seed=seed + 1), dtype=np.uint8)
    out = np.empty(nbytes + (8 << 20), dtype=np.uint8)
    at, members = 0, []
    while at < nbytes:
        kind = rng.random()
        size = int(2 ** rng.uniform(10, 22))
        if kind < 0.6 or not members:
            off = int(rng.integers(0, len(pool) - size))
            out[at:at + size] = pool[off:off + size]
        elif kind < 0.85:
            out[at:at + size] = rng.integers(0, 256, size=size, dtype=np.uint8)
        else:
            m0, msz = members[int(rng.integers(0, len(members)))]
            size = msz
            out[at:at + size] = out[m0:m0 + size]
        members.append((at, size))
        at += size
        pad = (-at) % 512
        out[at:at + pad] = 0
        at += pad
    return out[:nbytes].tobytes()


def stride_stream(nseg, seg_bytes, copy_bytes=None, seed=99):
    """S4 "stride" shape (BASELINE configs[3], scaled): `nseg` segments of noise (seed + segment index); in every
    4th segment the first `copy_bytes` (default a quarter) repeat the segment k segments earlier, k cycling
    through 1, 3, 7 -- long matches at a distance of whole segments."""
    copy_bytes = seg_bytes // 4 if copy_bytes is None else copy_bytes
    segs = [np.frombuffer(noise(seg_bytes, seed=seed + i), dtype=np.uint8).copy() for i in range(nseg)]
    ks = (1, 3, 7)
    j = 0
    for i in range(3, nseg, 4):
        k = ks[j % 3]
        j += 1
        if i - k >= 0:
            segs[i][:copy_bytes] = segs[i - k][:copy_bytes]
    return b"".join(s.tobytes() for s in segs)


def tar_like_device(nbytes, device, seed=5, pool_bytes=48 << 20, max_member_log2=22):
    """The S3 mix of tar_like_fast built directly in HBM (BASELINE configs[2] at its full 64 GiB does not fit the host's
    generators): text members are slices of one Zipf text pool at random offsets, noise members come from torch's
    generator on the device, 15 % are exact duplicates of earlier members; 512-byte aligned.  Deterministic for a given
    (nbytes, seed, torch version), NOT byte-identical to tar_like_fast (different noise generator): the oracle is run on
    a prefix copied back from the device.  Returns a uint8 tensor of nbytes bytes."""
    import torch
    rng = np.random.default_rng(seed)
    pool = torch.frombuffer(bytearray(zipf_text(pool_bytes, seed=seed + 1)), dtype=torch.uint8).to(device)
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    out = torch.empty(nbytes + (8 << 20), dtype=torch.uint8, device=device)
    at, members = 0, []
    while at < nbytes:
        kind = rng.random()
        size = int(2 ** rng.uniform(10, max_member_log2))
        if kind < 0.6 or not members:
            off = int(rng.integers(0, pool_bytes - size))
            out[at:at + size] = pool[off:off + size]
        elif kind < 0.85:
            out[at:at + size].random_(0, 256, generator=g)
        else:
            m0, msz = members[int(rng.integers(0, len(members)))]
            size = msz
            out[at:at + size] = out[m0:m0 + size].clone() if m0 + size > at else out[m0:m0 + size]
        members.append((at, size))
        at += size
        pad = (-at) % 512
        out[at:at + pad] = 0
        at += pad
    return out[:nbytes]


def noise_device(nbytes, device, seed=99):
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    out = torch.empty(nbytes, dtype=torch.uint8, device=device)
    for a in range(0, nbytes, 1 << 30):  # (slice-wise: random_ materialises temporaries of the slice's size)
        out[a:a + (1 << 30)].random_(0, 256, generator=g)
    return out


def stride_stream_device(nseg, seg_bytes, device, copy_bytes=None, seed=99):
    """stride_stream's shape built in HBM (BASELINE configs[3]: 1 GiB segments, every 4th repeats the first quarter of the
    segment 1, 3 or 7 segments earlier)."""
    copy_bytes = seg_bytes // 4 if copy_bytes is None else copy_bytes
    out = noise_device(nseg * seg_bytes, device, seed=seed)
    ks, j = (1, 3, 7), 0
    for i in range(3, nseg, 4):
        k = ks[j % 3]
        j += 1
        if i - k >= 0:
            out[i * seg_bytes:i * seg_bytes + copy_bytes] = out[(i - k) * seg_bytes:(i - k) * seg_bytes + copy_bytes]
    return out


# ---- reproducible streams: every byte a pure function of (seed, position) ---------------------------------------------
# The normative definition is in include/mrzgpu_synth.h and DESIGN.md section 4.9.  This is the host reference: numpy,
# integer arithmetic only, no code shared with the kernels of csrc/mrz_synth.hip, which must agree byte for byte.

_U = np.uint64
_SYN_G, _SYN_M1, _SYN_M2 = _U(0x9E3779B97F4A7C15), _U(0xBF58476D1CE4E5B9), _U(0x94D049BB133111EB)
(SYN_NOISE, SYN_WORD, SYN_VLEN, SYN_VCHAR, SYN_KIND, SYN_SIZE_E, SYN_SIZE_M, SYN_CSEED, SYN_DUP, SYN_VOCAB) = range(10)
SYN_VOCAB_WORDS, SYN_NEWLINE_EVERY, SYN_KIND_TEXT, SYN_KIND_NOISE = 5000, 20000, 0, 1
SYNTH_MEMBER = np.dtype([("dst", "<i8"), ("size", "<i8"), ("seed", "<u8"), ("kind", "<i4"), ("origin", "<i4")])


def _syn_mix(z):
    z = z ^ (z >> _U(30))
    z = z * _SYN_M1
    z = z ^ (z >> _U(27))
    z = z * _SYN_M2
    return z ^ (z >> _U(31))


def synth_rnd(seed, stream, i):
    """rnd(seed, stream, i) of the stream definition, for an array (or scalar) of counters i; uint64 array out."""
    with np.errstate(over="ignore"):
        key = _syn_mix(np.array([int(seed) & (2 ** 64 - 1)], dtype=_U) + _SYN_G * _U(stream + 1))
        i = np.atleast_1d(np.asarray(i)).astype(_U)
        return _syn_mix(key + _SYN_G * (i + _U(1)))


def synth_noise(nbytes, seed, start=0):
    """Bytes [start, start + nbytes) of noise(seed): byte j is byte j & 7 (little-endian) of rnd(seed, NOISE, j >> 3).
    Returns a uint8 array."""
    out = np.empty(nbytes, dtype=np.uint8)
    step = 1 << 27  # bytes per block of temporaries
    for a in range(0, nbytes, step):
        lo, hi = start + a, start + min(nbytes, a + step)
        w = synth_rnd(seed, SYN_NOISE, np.arange(lo >> 3, (hi + 7) >> 3, dtype=_U)).astype("<u8")
        out[a:a + hi - lo] = w.view(np.uint8)[lo - (lo >> 3 << 3):hi - (lo >> 3 << 3)]
    return out


_syn_cum = None


def synth_zipf_table():
    """cum[r] = sum over i <= r of floor(2^28 / (i + 1)), r < 5000: Zipf 1/rank in integers (uint32; cum[4999] ~ 2.44e9)."""
    global _syn_cum
    if _syn_cum is None:
        c = np.cumsum((1 << 28) // np.arange(1, SYN_VOCAB_WORDS + 1, dtype=np.int64))
        assert c[-1] < 1 << 32
        _syn_cum = c.astype(np.uint32)
    return _syn_cum


def synth_vocab(vocab_seed):
    """(lens, table): 5000 words of 2..10 letters a..z; table[w] holds word w, one separator space and padding (11 B)."""
    w = np.arange(SYN_VOCAB_WORDS, dtype=_U)
    lens = (2 + synth_rnd(vocab_seed, SYN_VLEN, w) % _U(9)).astype(np.int64)
    ch = (97 + synth_rnd(vocab_seed, SYN_VCHAR, np.arange(SYN_VOCAB_WORDS * 10, dtype=_U)) % _U(26)).astype(np.uint8)
    table = np.zeros((SYN_VOCAB_WORDS, 11), dtype=np.uint8)
    table[:, :10] = ch.reshape(SYN_VOCAB_WORDS, 10)
    table[np.arange(SYN_VOCAB_WORDS), lens] = 32
    return lens, table


def _syn_text_words(seed, k0, k1, cum, lens, table):
    """The bytes of words [k0, k1) of text(seed, .), separators included, as one uint8 array."""
    k = np.arange(k0, k1, dtype=_U)
    r = np.searchsorted(cum, (synth_rnd(seed, SYN_WORD, k) % _U(int(cum[-1]))).astype(np.uint32), side="right")
    rows = table[r]
    n = lens[r] + 1
    nl = np.nonzero((k + _U(1)) % _U(SYN_NEWLINE_EVERY) == 0)[0]
    rows[nl, n[nl] - 1] = 10
    return rows[np.arange(11)[None, :] < n[:, None]]


def synth_text(nbytes, seed, vocab_seed, _vocab=None):
    """The first nbytes of text(seed, vocab_seed): word k has rank r = the first r with cum[r] > rnd(seed, WORD, k) %
    cum[4999]; every word is followed by a space, every 20000th by a newline.  Returns a uint8 array."""
    cum = synth_zipf_table()
    lens, table = _vocab or synth_vocab(vocab_seed)
    out = np.empty(nbytes, dtype=np.uint8)
    at = k = 0
    while at < nbytes:
        nw = min(1 << 22, (nbytes - at) // 6 + 16)  # the mean word and its separator are ~ 7 bytes; short: go round again
        b = _syn_text_words(seed, k, k + nw, cum, lens, table)
        take = min(len(b), nbytes - at)
        out[at:at + take] = b[:take]
        at += take
        k += nw
    return out


def synth_tar_plan(nbytes, seed):
    """The members of tar(seed) that begin before nbytes, as a SYNTH_MEMBER array (what mrz_synth_tar takes): member m
    draws kind = rnd % 100 and size = (1 << e) + rnd % (1 << e), e = 10 + rnd % 12.  kind < 60 (or m == 0): text with a
    seed of its own; < 85: noise with a seed of its own; else a duplicate of member rnd % m, which carries its original's
    kind, size and seed (`origin` = the original's index, -1 for a member that is no duplicate).  dst = the member's
    offset; every member is zero-padded to a multiple of 512."""
    parts, at, m0 = [], 0, 0
    kinds, sizes, seeds, origin = [], [], [], []
    while at < nbytes:
        nm = max(64, int((nbytes - at) / 400e3))  # the mean member is ~ 560 KB
        m = np.arange(m0, m0 + nm, dtype=_U)
        kd = (synth_rnd(seed, SYN_KIND, m) % _U(100)).astype(np.int64)
        e = _U(10) + synth_rnd(seed, SYN_SIZE_E, m) % _U(12)
        sz = ((_U(1) << e) + synth_rnd(seed, SYN_SIZE_M, m) % (_U(1) << e)).astype(np.int64)
        cs = synth_rnd(seed, SYN_CSEED, m)
        dp = synth_rnd(seed, SYN_DUP, m)
        for i in range(nm):
            if at >= nbytes:
                break
            mi = m0 + i
            if kd[i] < 60 or mi == 0:
                rec = (SYN_KIND_TEXT, int(sz[i]), int(cs[i]), -1)
            elif kd[i] < 85:
                rec = (SYN_KIND_NOISE, int(sz[i]), int(cs[i]), -1)
            else:
                j = int(dp[i] % _U(mi))
                o = origin[j] if origin[j] >= 0 else j
                rec = (kinds[o], sizes[o], seeds[o], o)
            kinds.append(rec[0]); sizes.append(rec[1]); seeds.append(rec[2]); origin.append(rec[3])
            parts.append(at)
            at += (rec[1] + 511) & ~511
        m0 += nm
    plan = np.zeros(len(parts), dtype=SYNTH_MEMBER)
    plan["dst"], plan["size"], plan["seed"], plan["kind"], plan["origin"] = parts, sizes, seeds, kinds, origin
    return plan


def synth_tar_vocab_seed(seed):
    """The seed of the one vocabulary all text members of tar(seed) share."""
    return int(synth_rnd(seed, SYN_VOCAB, 0)[0])


def synth_tar(nbytes, seed, start=0, plan=None):
    """Bytes [start, start + nbytes) of tar(seed), S3 as SURVEY section 8d specifies it (fresh text per text member).
    Every member is regenerated from its descriptor, duplicates included, so a range needs none of the bytes before it.
    Returns a uint8 array."""
    if plan is None:
        plan = synth_tar_plan(start + nbytes, seed)
    vocab = synth_vocab(synth_tar_vocab_seed(seed))
    out = np.zeros(nbytes, dtype=np.uint8)
    end = start + nbytes
    for d in plan:
        dst, size = int(d["dst"]), int(d["size"])
        lo, hi = max(dst, start), min(dst + size, end)
        if lo >= hi:
            continue
        if d["kind"] == SYN_KIND_NOISE:
            out[lo - start:hi - start] = synth_noise(hi - lo, int(d["seed"]), start=lo - dst)
        else:
            out[lo - start:hi - start] = synth_text(hi - dst, int(d["seed"]), None, _vocab=vocab)[lo - dst:]
    return out


def _synth_device(nbytes, device, lib, ctx, fill):
    """torch allocates nbytes on `device` (a cuda device; "cpu" with the test emulator's library), fill(ctx, out) has the
    library write them.  ctx: an open RzipContext to use instead of a temporary one."""
    import torch
    from . import binding
    dev = torch.device(device)
    out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if ctx is not None:
        fill(ctx, out)
        return out
    index = dev.index if dev.type == "cuda" and dev.index is not None else 0
    with binding.RzipContext(level=1, device=index, lib=lib) as tmp:
        fill(tmp, out)
    return out


def synth_noise_device(nbytes, device, seed, start=0, lib=None, ctx=None):
    """synth_noise(nbytes, seed, start) built by the HIP kernels in device memory: a uint8 torch tensor."""
    return _synth_device(nbytes, device, lib, ctx, lambda c, out: c.synth_noise(out, nbytes, seed, start=start))


def synth_text_device(nbytes, device, seed, vocab_seed, lib=None, ctx=None):
    """synth_text(nbytes, seed, vocab_seed) built by the HIP kernels in device memory: a uint8 torch tensor."""
    return _synth_device(nbytes, device, lib, ctx, lambda c, out: c.synth_text(out, nbytes, seed, vocab_seed))


def synth_tar_device(nbytes, device, seed, start=0, lib=None, ctx=None, plan=None):
    """synth_tar(nbytes, seed, start) built by the HIP kernels in device memory: a uint8 torch tensor.  The plan is made
    on the host (synth_tar_plan); any byte range can be built on any rank without the bytes before it."""
    if plan is None:
        plan = synth_tar_plan(start + nbytes, seed)
    vs = synth_tar_vocab_seed(seed)
    return _synth_device(nbytes, device, lib, ctx, lambda c, out: c.synth_tar(out, nbytes, plan, vs, start=start))
