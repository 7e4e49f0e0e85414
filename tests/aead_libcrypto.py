"""The system libcrypto (OpenSSL 3) through ctypes, as the second opinion on
aead_ref.py: ChaCha20-Poly1305 (IETF) from EVP_chacha20_poly1305, and
XChaCha20-Poly1305 by composition -- HChaCha20 is the raw EVP_chacha20 keystream
block minus the input state words (the block function adds the state to the
rounds' output, HChaCha20 is that output), then the IETF AEAD with the subkey.
``load()`` returns None where libcrypto cannot be loaded."""
import ctypes
import ctypes.util

import numpy as np

_CTRL_SET_IVLEN, _CTRL_GET_TAG, _CTRL_SET_TAG = 0x9, 0x10, 0x11


class LibCrypto:
    def __init__(self, L):
        self.L = L
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.EVP_CIPHER_CTX_new.restype = vp
        L.EVP_CIPHER_CTX_free.argtypes = [vp]
        for name in ("EVP_chacha20_poly1305", "EVP_chacha20"):
            getattr(L, name).restype = vp
        for name in ("EVP_EncryptInit_ex", "EVP_DecryptInit_ex"):
            getattr(L, name).argtypes = [vp, vp, vp, ctypes.c_char_p, ctypes.c_char_p]
        for name in ("EVP_EncryptUpdate", "EVP_DecryptUpdate"):
            getattr(L, name).argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ci), ctypes.c_char_p, ci]
        for name in ("EVP_EncryptFinal_ex", "EVP_DecryptFinal_ex"):
            getattr(L, name).argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ci)]
        L.EVP_CIPHER_CTX_ctrl.argtypes = [vp, ci, ci, ctypes.c_char_p]

    def _ok(self, rc):
        if rc != 1:
            raise RuntimeError("libcrypto call failed")

    def chacha20_stream(self, key, iv16, n):
        """n keystream bytes of EVP_chacha20; iv16 = le32(counter) || nonce(12)."""
        L = self.L
        c = L.EVP_CIPHER_CTX_new()
        try:
            self._ok(L.EVP_EncryptInit_ex(c, L.EVP_chacha20(), None, key, iv16))
            out = ctypes.create_string_buffer(n + 64)
            outl = ctypes.c_int()
            self._ok(L.EVP_EncryptUpdate(c, out, ctypes.byref(outl), bytes(n), n))
            return out.raw[:outl.value]
        finally:
            L.EVP_CIPHER_CTX_free(c)

    def hchacha20(self, key, nonce16):
        block = np.frombuffer(self.chacha20_stream(key, nonce16, 64), dtype="<u4")
        state = np.frombuffer(b"expand 32-byte k" + key + nonce16, dtype="<u4")
        x = block - state  # (mod 2^32)
        return np.concatenate([x[0:4], x[12:16]]).astype("<u4").tobytes()

    def ietf_seal(self, key, nonce12, pt):
        L = self.L
        c = L.EVP_CIPHER_CTX_new()
        try:
            self._ok(L.EVP_EncryptInit_ex(c, L.EVP_chacha20_poly1305(), None, None, None))
            self._ok(L.EVP_CIPHER_CTX_ctrl(c, _CTRL_SET_IVLEN, 12, None))
            self._ok(L.EVP_EncryptInit_ex(c, None, None, key, nonce12))
            out = ctypes.create_string_buffer(len(pt) + 64)
            outl, fin = ctypes.c_int(), ctypes.c_int()
            self._ok(L.EVP_EncryptUpdate(c, out, ctypes.byref(outl), pt, len(pt)))
            self._ok(L.EVP_EncryptFinal_ex(c, ctypes.cast(ctypes.byref(out, outl.value), ctypes.c_char_p),
                                           ctypes.byref(fin)))
            tag = ctypes.create_string_buffer(16)
            self._ok(L.EVP_CIPHER_CTX_ctrl(c, _CTRL_GET_TAG, 16, tag))
            return out.raw[:outl.value + fin.value] + tag.raw
        finally:
            L.EVP_CIPHER_CTX_free(c)

    def ietf_open(self, key, nonce12, sealed):
        """-> the plaintext, or None if the tag does not match."""
        L = self.L
        ct, tag = sealed[:-16], sealed[-16:]
        c = L.EVP_CIPHER_CTX_new()
        try:
            self._ok(L.EVP_DecryptInit_ex(c, L.EVP_chacha20_poly1305(), None, None, None))
            self._ok(L.EVP_CIPHER_CTX_ctrl(c, _CTRL_SET_IVLEN, 12, None))
            self._ok(L.EVP_DecryptInit_ex(c, None, None, key, nonce12))
            out = ctypes.create_string_buffer(len(ct) + 64)
            outl, fin = ctypes.c_int(), ctypes.c_int()
            self._ok(L.EVP_DecryptUpdate(c, out, ctypes.byref(outl), ct, len(ct)))
            self._ok(L.EVP_CIPHER_CTX_ctrl(c, _CTRL_SET_TAG, 16, tag))
            if L.EVP_DecryptFinal_ex(c, ctypes.cast(ctypes.byref(out, outl.value), ctypes.c_char_p),
                                     ctypes.byref(fin)) != 1:
                return None
            return out.raw[:outl.value + fin.value]
        finally:
            L.EVP_CIPHER_CTX_free(c)

    def xseal(self, key, nonce24, pt):
        """-> the record nonce || ciphertext || tag."""
        sub = self.hchacha20(key, nonce24[:16])
        return nonce24 + self.ietf_seal(sub, bytes(4) + nonce24[16:], pt)

    def xopen(self, key, record):
        sub = self.hchacha20(key, record[:16])
        return self.ietf_open(sub, bytes(4) + record[16:24], record[24:])


def load():
    name = ctypes.util.find_library("crypto")
    if not name:
        return None
    try:
        L = ctypes.CDLL(name)
        lc = LibCrypto(L)
        lc.ietf_seal(bytes(32), bytes(12), b"")
        return lc
    except (OSError, AttributeError, RuntimeError):
        return None
