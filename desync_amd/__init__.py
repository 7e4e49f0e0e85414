"""desync_amd -- MI355X-native content-defined chunker (desync drop-in).

The chunking hot path of folbricht/desync (chunker.go Buzhash scan + cut
chain, make.go split-and-align) runs as hand-written gfx950 HIP kernels in
libdsx.so behind the C ABI of include/dsx.h.  This package is the host-side
mirror of the reference's Go API for that path:

    NewChunker / Chunker.Next / Advance / Min / Avg / Max   (chunker.go)
    NewHash / Hash (the exported legacy rolling hash)       (chunker.go:320-371)
    IndexFromFile, ChunkingStats                            (make.go)
    VerifyIndex                                             (verifyindex.go)
    ChunkStream, ChunkStorage                               (index.go, chunkstorage.go)
    ChopFile, ChunkInvalid                                  (chop.go, errors.go)
    Index, IndexChunk, Index.WriteTo, IndexFromReader       (index.go)
    Digest (SHA512256 / SHA256), NullChunk                  (digest.go)
    Info, IDSet, dedup (chunk-ID sets on the GPU)           (cmd/desync/info.go, fileseed.go)
    NewIndexSeed, NewSeedSequencer, Plan, AssembleBlob      (fileseed.go, sequencer.go, assemble.go)
    DeviceStore, ChopBlob, ChunkMissing (a chunk store in HBM)  (store.go, local.go, chop.go, errors.go)
    IndexFromBlobs, ChopBlobs, cut_device_many (many blobs per call)  (make.go, chop.go)
    chunk_ids_known, DeviceStore.chunk_ids (IDs by comparison with the store)  (make.go:223, chunkstorage.go:44-67)
    DeviceStore.Prune, RemoveChunk, Verify(repair=True)     (local.go, cmd/desync/prune.go)
    NewXChaCha20Poly1305, Converters, Compressor, StoreOptions  (encrypt.go, converter.go, store.go)
    DeviceStore.Seal, PutSealed, WriteLocal, ReadLocal      (encrypt.go, local.go)
    Copy, Cache, NewCache, DeviceStore.CopyFrom, Grow       (copy.go, cache.go)
    DeviceStore(track=, evict=), Track, Touch, Evict, stamps  (least recently used eviction; no reference counterpart)
    NewIndexReadSeeker, IndexPos, Cat, read_ranges, DeviceIndex  (readseeker.go, cmd/desync/cat.go)

There is no CPU fallback: without libdsx.so or a GPU, calls raise.
"""
from .chunker import ChunkerReadError, ChunkerWindowSize, Chunker, NewChunker, Params  # noqa: F401
from .digest import SHA256, SHA512256, NewNullChunk, NullChunk, set_digest  # noqa: F401
from .errors import ChunkInvalid, ChunkMissing, Interrupted  # noqa: F401
from .index import FormatIndex, Index, IndexChunk, IndexFromReader  # noqa: F401
from .stream import Chunk, ChunkStorage, ChunkStream, MemoryStore  # noqa: F401
from .make import ChunkingStats, IndexFromBlobs, IndexFromFile, VerifyError, cut_device_many, VerifyIndex, chunk_ids, cut_device, cut_device_result, \
    cut_fd, cut_host, file_size, ids_fd, ids_host, index_fd, index_host  # noqa: F401
from .chop import ChopFile  # noqa: F401
from .hash import Hash, NewHash  # noqa: F401
from .info import IDSet, Info, dedup  # noqa: F401
from .extract import AssembleBlob, IndexSeed, NewIndexSeed, NewSeedSequencer, Plan, SeedInvalid, SeedSequencer, \
    Segment, StorageError  # noqa: F401
from .store import ChopBlob, ChopBlobs, DeviceStore, chunk_ids_known  # noqa: F401
from .copy import Cache, Copy, NewCache  # noqa: F401
from .readseeker import Cat, DeviceIndex, IndexPos, NewIndexReadSeeker, read_ranges  # noqa: F401
from .encrypt import AEADConverter, AuthenticationError, Compressor, Converters, EncryptionKeySize, NewAES256GCM, \
    NewXChaCha20Poly1305, StoreOptions  # noqa: F401

__all__ = [
    "ChunkerWindowSize", "Chunker", "ChunkerReadError", "NewChunker", "Params", "SHA256", "SHA512256", "NullChunk",
    "NewNullChunk", "set_digest", "Interrupted", "FormatIndex", "Index", "IndexChunk",
    "IndexFromReader", "Chunk", "ChunkStorage", "ChunkStream", "MemoryStore", "ChunkingStats", "IndexFromFile", "cut_device", "cut_device_result",
    "cut_fd", "cut_host", "chunk_ids", "VerifyIndex", "VerifyError", "file_size", "index_fd",
    "index_host", "ids_fd", "ids_host", "ChopFile", "ChunkInvalid", "Hash", "NewHash",
    "IDSet", "Info", "dedup",
    "NewIndexSeed", "IndexSeed", "NewSeedSequencer", "SeedSequencer", "Plan", "Segment", "SeedInvalid",
    "AssembleBlob", "DeviceStore", "ChopBlob", "ChunkMissing", "Copy", "Cache", "NewCache",
    "EncryptionKeySize", "NewXChaCha20Poly1305", "NewAES256GCM", "AEADConverter", "Compressor", "Converters",
    "StoreOptions", "AuthenticationError", "IndexFromBlobs", "ChopBlobs", "cut_device_many", "chunk_ids_known",
    "StorageError", "NewIndexReadSeeker", "IndexPos", "Cat", "read_ranges", "DeviceIndex",
]
