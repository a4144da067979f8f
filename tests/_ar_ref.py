"""An independent Python restatement of what `ar-mrzip` does to a list of members (ar-mrzip/ar-mrzip.cpp:137-172,
395-532), for the tests of mrz_tlsh_batch / mrz_ar_order / mrz_ar_create: the TLSH digest (256 buckets, 3 checksum
bytes), the 137-byte stored form, the greedy similarity order, the duplicate collapse and the ARZIP framing.  The
`ar-mrzip` binary itself does not build with the compilers at hand, so the order, the collapse and the framing are
pinned against this file; the digest is pinned against the reference library's own strings (tests/golden/tlsh.json),
and tlsh() below is checked against them too.  Also the seeded inputs that the fixture and the tests share."""
import hashlib
import struct

import numpy as np

from tests import _util

STORED = 137
ZERO = bytes(STORED)

PEARSON = bytes([
    1, 87, 49, 12, 176, 178, 102, 166, 121, 193, 6, 84, 249, 230, 44, 163, 14, 197, 213, 181, 161, 85, 218, 80, 64, 239,
    24, 226, 236, 142, 38, 200, 110, 177, 104, 103, 141, 253, 255, 50, 77, 101, 81, 18, 45, 96, 31, 222, 25, 107, 190,
    70, 86, 237, 240, 34, 72, 242, 20, 214, 244, 227, 149, 235, 97, 234, 57, 22, 60, 250, 82, 175, 208, 5, 127, 199, 111,
    62, 135, 248, 174, 169, 211, 58, 66, 154, 106, 195, 245, 171, 17, 187, 182, 179, 0, 243, 132, 56, 148, 75, 128, 133,
    158, 100, 130, 126, 91, 13, 153, 246, 216, 219, 119, 68, 223, 78, 83, 88, 201, 99, 122, 11, 92, 32, 136, 114, 52, 10,
    138, 30, 48, 183, 156, 35, 61, 26, 143, 74, 251, 94, 129, 162, 63, 152, 170, 7, 115, 167, 241, 206, 3, 150, 55, 59,
    151, 220, 90, 53, 23, 131, 125, 173, 15, 238, 79, 95, 89, 16, 105, 137, 225, 224, 217, 160, 37, 123, 118, 73, 2, 157,
    46, 116, 9, 145, 134, 228, 207, 212, 202, 215, 69, 229, 27, 188, 67, 124, 168, 252, 42, 4, 29, 108, 21, 247, 19, 205,
    39, 203, 233, 40, 186, 147, 198, 192, 155, 33, 164, 191, 98, 204, 165, 180, 117, 76, 140, 36, 210, 172, 41, 54, 159,
    8, 185, 232, 113, 196, 231, 47, 146, 120, 51, 65, 28, 144, 254, 221, 93, 189, 194, 139, 112, 43, 71, 109, 184, 209])


def _swap(b):
    return ((b << 4) | (b >> 4)) & 255


def tlsh(data, min_len, len_code):
    """The 138 hex characters, or "" where the reference gives none.  min_len: the smallest length of every length
    code (tlsh.json "lvalue_min_len"); len_code: unused unless given (a callable length -> code)."""
    n = len(data)
    if n < 50:
        return ""
    v = np.frombuffer(PEARSON, dtype=np.uint8)
    d = np.frombuffer(data, dtype=np.uint8)
    cur, b1, b2, b3, b4 = d[4:], d[3:-1], d[2:-2], d[1:-3], d[:-4]
    counts = np.zeros(256, dtype=np.int64)
    for salt, x, y in ((49, b1, b2), (12, b1, b3), (178, b2, b3), (166, b2, b4), (84, b1, b4), (230, b3, b4)):
        counts += np.bincount(v[v[v[salt ^ cur] ^ x] ^ y], minlength=256)
    counts &= 0xFFFFFFFF
    a0 = v[v[1 ^ cur] ^ b1].tolist()
    curl, b1l, p = cur.tolist(), b1.tolist(), PEARSON
    c0 = c1 = c2 = 0
    for a, di, dj in zip(a0, curl, b1l):
        c0 = p[a ^ c0]
        c1 = p[p[p[p[c0] ^ di] ^ dj] ^ c1]
        c2 = p[p[p[p[c1] ^ di] ^ dj] ^ c2]
    srt = np.sort(counts)
    q1, q2, q3 = int(srt[63]), int(srt[127]), int(srt[191])
    if q3 == 0 or int((counts > 0).sum()) <= 128:
        return ""
    code = []
    for i in range(64):
        h = 0
        for j in range(4):
            k = int(counts[4 * i + j])
            h |= (3 if k > q3 else 2 if k > q2 else 1 if k > q1 else 0) << (2 * j)
        code.append(h)
    lv = len_code(n) if len_code else max(i for i, m in enumerate(min_len) if m <= n)
    r1 = int(np.float32((q1 * 100) & 0xFFFFFFFF) / np.float32(q3)) % 16
    r2 = int(np.float32((q2 * 100) & 0xFFFFFFFF) / np.float32(q3)) % 16
    raw = bytes([_swap(c0), _swap(c1), _swap(c2), _swap(lv), _swap(r1 | (r2 << 4))] + code[::-1])
    return raw.hex().upper()


def stored_digest(hex138, size):
    """What the archive keeps: 137 of the 138 characters, or zeros for a small member or one without a digest"""
    if size <= 500 or not hex138:
        return ZERO
    return hex138.encode()[:STORED]


def score(a, b):
    return sum(x == y for x, y in zip(a, b))


def order(digests):
    """The greedy order over 137-byte digests: the permutation (indices into `digests`)"""
    perm = list(range(len(digests)))
    n = len(perm)
    arr = [np.frombuffer(bytes(x), dtype=np.uint8) for x in digests]
    c = 0
    while c + 1 < n:
        best, nxt = 0, 0
        head = arr[perm[c]]
        for i in range(c + 1, n):
            s = int((head == arr[perm[i]]).sum())
            if s > 130:
                nxt = i
                break
            if s > best:
                best, nxt = s, i
        perm[c + 1], perm[nxt] = perm[nxt], perm[c + 1]
        c += 1
    return perm


def create(members, digests):
    """members: (name bytes, mtime, data bytes) in the caller's order; digests: their stored 137 bytes.  Returns
    (archive bytes, records in archive order as dicts)."""
    perm = order(digests)
    recs, seen, off = [], {}, 0
    for i in perm:
        name, mtime, data = members[i]
        sum_ = hashlib.blake2b(data).digest()
        if sum_ not in seen:
            seen[sum_] = off
            off += len(data)
        recs.append({"index": i, "name": name, "mtime": mtime, "size": len(data), "offset": seen[sum_],
                     "checksum": sum_, "digest": digests[i], "data": data})
    meta = b"".join(struct.pack(">QQQ", r["mtime"], r["size"], r["offset"]) + r["checksum"] + r["digest"] +
                    struct.pack(">I", len(r["name"])) + r["name"] for r in recs)
    assert len(meta) == sum(len(r["name"]) + 88 + 4 + STORED for r in recs)
    out, at = bytearray(b"ARZIP" + struct.pack(">Q", len(meta)) + meta), 0
    for r in recs:
        if r["offset"] == at:
            out += r["data"]
            at += r["size"]
    return bytes(out), recs


# ---- seeded inputs shared by tests/golden/make_tlsh_golden.py and the tests ---------------------------------------

KINDS = ("noise", "text", "alpha4", "const", "bytes256")
SEGMENTS = (64, 256)
LENGTHS = sorted({0, 4, 5, 49, 50, 255, 501, 502, 4095, 4096, 4097} |
                 {x for s in SEGMENTS for x in (s - 1, s, s + 1, s + 4, 2 * s + 3, 5 * s + 1)})


def make_input(kind, n, seed=0):
    if kind == "noise":
        return _util.xorshift_noise(n, seed=1000 + seed + n)
    if kind == "text":
        t = _util.zipf_text(4200, seed=11 + seed)
        return (t * (n // len(t) + 1))[:n]
    if kind == "alpha4":
        rng = np.random.default_rng(77 + seed + n)
        return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)])
    if kind == "const":
        return bytes([0x5A]) * n
    if kind == "bytes256":
        return (bytes(range(256)) * (n // 256 + 1))[:n]
    raise ValueError(kind)


def small_inputs():
    """name -> bytes, every kind at every length"""
    return {"%s_%d" % (k, n): make_input(k, n) for k in KINDS for n in LENGTHS}


def big_member():
    """8 MiB over a 64-symbol alphabet"""
    rng = np.random.default_rng(8)
    return (rng.integers(0, 64, size=8 << 20, dtype=np.uint8) + 48).astype(np.uint8).tobytes()


def mixed_batch():
    """300 members of mixed kinds and sizes from 0 bytes to about 180 KB"""
    rng = np.random.default_rng(300)
    out = []
    for i in range(300):
        n = int(2 ** rng.uniform(0, 17.5)) - 1
        out.append(make_input(KINDS[i % len(KINDS)], n, seed=i))
    return out


def threshold_message(n):
    """a message of n bytes that has a digest (n >= 50)"""
    return _util.xorshift_noise(n, seed=4242)
