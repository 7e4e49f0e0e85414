"""A CPU reference of the AEAD store converter (encrypt.go): XChaCha20-Poly1305
as golang.org/x/crypto/chacha20poly1305's NewX(key).Seal(out, nonce, in, nil)
computes it, with ChaCha20 and HChaCha20 in numpy (every block of a message at
once) and Poly1305 in Python integers.  The GPU tests compare every byte with
it; test_aead_host.py pins it against libcrypto and tests/golden/aead_vectors.json.

A record is nonce(24) || ciphertext || tag(16)."""
import numpy as np

NONCE = 24
TAG = 16
OVERHEAD = NONCE + TAG
P1305 = (1 << 130) - 5
CLAMP = 0x0ffffffc0ffffffc0ffffffc0fffffff
_CONSTS = np.frombuffer(b"expand 32-byte k", dtype="<u4")


class AuthError(Exception):
    """chacha20poly1305's ErrOpen."""

    def __init__(self):
        super().__init__("chacha20poly1305: message authentication failed")


def _rotl(x, n):
    return (x << np.uint32(n)) | (x >> np.uint32(32 - n))


def _rounds(x):
    """20 rounds over the columns of x (16, nblocks) uint32, in place."""
    def qr(a, b, c, d):
        x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 16)
        x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 12)
        x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 8)
        x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 7)
    for _ in range(10):
        qr(0, 4, 8, 12), qr(1, 5, 9, 13), qr(2, 6, 10, 14), qr(3, 7, 11, 15)
        qr(0, 5, 10, 15), qr(1, 6, 11, 12), qr(2, 7, 8, 13), qr(3, 4, 9, 14)
    return x


def chacha20_blocks(key, counter, nonce12, nblocks):
    """The keystream blocks counter .. counter + nblocks - 1 (RFC 8439 2.3) as bytes."""
    st = np.empty((16, nblocks), dtype=np.uint32)
    st[0:4] = _CONSTS[:, None]
    st[4:12] = np.frombuffer(key, dtype="<u4")[:, None]
    st[12] = (counter + np.arange(nblocks, dtype=np.uint64)).astype(np.uint32)
    st[13:16] = np.frombuffer(nonce12, dtype="<u4")[:, None]
    with np.errstate(over="ignore"):
        out = _rounds(st.copy()) + st
    return np.ascontiguousarray(out.T).astype("<u4").tobytes()


def hchacha20(key, nonce16):
    """draft-irtf-cfrg-xchacha 2.2: words 0-3 and 12-15 after the rounds, no final sum."""
    st = np.empty((16, 1), dtype=np.uint32)
    st[0:4] = _CONSTS[:, None]
    st[4:12] = np.frombuffer(key, dtype="<u4")[:, None]
    st[12:16] = np.frombuffer(nonce16, dtype="<u4")[:, None]
    with np.errstate(over="ignore"):
        x = _rounds(st)
    return np.concatenate([x[0:4, 0], x[12:16, 0]]).astype("<u4").tobytes()


def chacha20_xor(key, counter, nonce12, data):
    if not data:
        return b""
    ks = chacha20_blocks(key, counter, nonce12, (len(data) + 63) // 64)
    a = np.frombuffer(data, dtype=np.uint8)
    return (a ^ np.frombuffer(ks, dtype=np.uint8)[:len(a)]).tobytes()


def poly1305(otk, msg):
    """RFC 8439 2.5: the tag of msg under the one-time key otk = r || s."""
    r = int.from_bytes(otk[:16], "little") & CLAMP
    s = int.from_bytes(otk[16:32], "little")
    h = 0
    for i in range(0, len(msg), 16):
        blk = msg[i:i + 16]
        h = (h + int.from_bytes(blk, "little") + (1 << (8 * len(blk)))) * r % P1305
    return ((h + s) & ((1 << 128) - 1)).to_bytes(16, "little")


def _mac_data(ct):
    """The AEAD's MAC input with empty additional data (RFC 8439 2.8)."""
    return ct + bytes(-len(ct) % 16) + (0).to_bytes(8, "little") + len(ct).to_bytes(8, "little")


def ietf_seal(key, nonce12, pt):
    """ChaCha20-Poly1305 (RFC 8439 2.8), empty AAD -> ciphertext || tag."""
    otk = chacha20_blocks(key, 0, nonce12, 1)[:32]
    ct = chacha20_xor(key, 1, nonce12, pt)
    return ct + poly1305(otk, _mac_data(ct))


def ietf_open(key, nonce12, sealed):
    if len(sealed) < TAG:
        raise AuthError()
    ct, tag = sealed[:-TAG], sealed[-TAG:]
    otk = chacha20_blocks(key, 0, nonce12, 1)[:32]
    want = poly1305(otk, _mac_data(ct))
    if want != tag:
        raise AuthError()
    return chacha20_xor(key, 1, nonce12, ct)


def _x(key, nonce24):
    return hchacha20(key, nonce24[:16]), bytes(4) + nonce24[16:24]


def seal(key, nonce, pt):
    """-> the record nonce || ciphertext || tag (aeadConverter.toStorage with this nonce)."""
    assert len(key) == 32 and len(nonce) == NONCE
    sub, n12 = _x(bytes(key), bytes(nonce))
    return bytes(nonce) + ietf_seal(sub, n12, bytes(pt))


def open(key, record):  # noqa: A001  (the issue's name for it)
    """aeadConverter.fromStorage: the plaintext, or ValueError / AuthError with the
    reference's messages."""
    record = bytes(record)
    if len(record) < NONCE:
        raise ValueError("no nonce prefix found in chunk, not encrypted or wrong algorithm")
    sub, n12 = _x(bytes(key), record[:NONCE])
    return ietf_open(sub, n12, record[NONCE:])


def seal_many(key, nonces, blob, ends, start=0):
    """What dsx_aead_seal writes: the records of the chunks [start, ends[0]),
    [ends[0], ends[1]), ... of blob, concatenated, and their ends.  The same
    construction as seal(), with the cipher blocks of all records in one numpy
    pass (test_aead_host.py holds the two against each other)."""
    n = len(ends)
    if not n:
        return b"", np.empty(0, dtype=np.uint64)
    nonces = np.frombuffer(bytes(nonces), dtype=np.uint8).reshape(n, NONCE)
    bounds = np.concatenate([[int(start)], np.asarray(ends, dtype=np.int64)])
    sizes = np.diff(bounds)
    nw = np.ascontiguousarray(nonces).view("<u4").astype(np.uint32)  # (n, 6)
    st = np.empty((16, n), dtype=np.uint32)
    st[0:4] = _CONSTS[:, None]
    st[4:12] = np.frombuffer(key, dtype="<u4")[:, None]
    st[12:16] = nw[:, 0:4].T
    with np.errstate(over="ignore"):
        x = _rounds(st)
    sub = np.concatenate([x[0:4], x[12:16]])  # (8, n)
    nblk = (sizes + 63) // 64 + 1             # block 0: the one-time key
    rec = np.repeat(np.arange(n), nblk)
    first = np.concatenate([[0], np.cumsum(nblk)[:-1]])
    st = np.empty((16, rec.size), dtype=np.uint32)
    st[0:4] = _CONSTS[:, None]
    st[4:12] = sub[:, rec]
    st[12] = (np.arange(rec.size) - first[rec]).astype(np.uint32)
    st[13] = 0
    st[14:16] = nw[rec, 4:6].T
    with np.errstate(over="ignore"):
        ks = _rounds(st.copy()) + st
    ks = np.ascontiguousarray(ks.T).astype("<u4").view(np.uint8).reshape(-1, 64)
    data = np.frombuffer(bytes(blob), dtype=np.uint8)
    out = []
    for i in range(n):
        otk = ks[first[i], :32].tobytes()
        stream = ks[first[i] + 1:first[i] + nblk[i]].reshape(-1)[:sizes[i]]
        ct = (data[bounds[i]:bounds[i + 1]] ^ stream).tobytes()
        out.append(nonces[i].tobytes() + ct + poly1305(otk, _mac_data(ct)))
    return b"".join(out), np.cumsum(sizes + OVERHEAD).astype(np.uint64)
