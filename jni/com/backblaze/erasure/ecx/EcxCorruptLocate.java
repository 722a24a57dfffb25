package com.backblaze.erasure.ecx;

/**
 * The step between the scrub and the repair: which shard is corrupt in each stripe that fails
 * ReedSolomon.isParityCorrect (ReedSolomon.java:129-178), over many DEVICE-resident stripes at
 * once, on libecx.so.  The reference has no counterpart.  Read-only on the stripes; the answers are
 * device arrays, so an EcxMixedDecode built from the shards' single-loss patterns in shard order
 * (pattern j: only shard j missing) heals the batch from {@code healId} on the same stream with no
 * host round trip.  With two parity shards, two corrupt shards at the same byte position can
 * imitate a third one; with three or more a code of distance m + 1 tells two errors from one.
 * (EcxParityCheck stays the host-memory scrub: its buffers carry a capacity to check, a device
 * address does not.)
 */
public final class EcxCorruptLocate {
    private long rs;  // 0 once closed
    private final int shardCount;
    private final int parityCount;

    /** The codec of ReedSolomon.create(dataShards, parityShards); 2 to 8 parity shards. */
    public EcxCorruptLocate(int dataShards, int parityShards) {
        if (parityShards < 2 || parityShards > 8) {
            throw new IllegalArgumentException("locate takes codes with 2 to 8 parity shards");
        }
        this.rs = Ecx.createReedSolomon(dataShards, parityShards);
        this.shardCount = dataShards + parityShards;
        this.parityCount = parityShards;
    }

    /** The single-loss patterns in shard order: what to build the healing EcxMixedDecode from. */
    public boolean[][] singleLossPatterns() {
        boolean[][] p = new boolean[shardCount][shardCount];
        for (int j = 0; j < shardCount; ++j) {
            for (int i = 0; i < shardCount; ++i) {
                p[j][i] = i != j;
            }
        }
        return p;
    }

    /**
     * ecx_rs_locate_corrupt_batch: stripe s's shard i at base + s * stripeStride + i * shardStride,
     * bytes [firstByte, firstByte + byteCount).  {@code suspect} (device bytes, nstripes * shards)
     * receives 1 where replacing that shard alone can make the stripe pass; {@code culprit} (device
     * ints, nstripes) -1 for a clean stripe, j for exactly one suspect, -2 when no single shard
     * explains the stripe; {@code healId} (device bytes, nstripes; 0 = not wanted) j or 255.  Only
     * enqueues on {@code stream} (0 = the default); the first call on a device must run outside
     * stream capture.
     */
    public void locateCorrupt(long base, long stripeStride, long shardStride, long nstripes, long firstByte,
                              long byteCount, long suspect, long culprit, long healId, long stream) {
        checkArguments(nstripes, byteCount, base, suspect, culprit, healId);
        if (stripeStride < 0 || shardStride < 0 || firstByte < 0) {
            throw new IllegalArgumentException("negative stride or first byte");
        }
        Ecx.check(EcxNative.rsLocateCorruptBatch(handle(), base, stripeStride, shardStride, nstripes, firstByte,
                byteCount, suspect, culprit, healId, stream));
    }

    /**
     * locateCorrupt over nstripes device-resident stripes in the blocked layout (EcxBlockedStripes),
     * over bytes [0, byteCount) of the natural shards (ecx_rs_locate_corrupt_blocked_batch);
     * blockBytes 0 = the recommended block.  {@code healId} feeds
     * EcxMixedDecode.decodeMissingBlockedBatch.
     */
    public void locateCorruptBlocked(long base, long nstripes, long byteCount, long blockBytes, long suspect,
                                     long culprit, long healId, long stream) {
        checkArguments(nstripes, byteCount, base, suspect, culprit, healId);
        if (blockBytes < 0) {
            throw new IllegalArgumentException("negative block size");
        }
        Ecx.check(EcxNative.rsLocateCorruptBlockedBatch(handle(), base, nstripes, byteCount, blockBytes, suspect,
                culprit, healId, stream));
    }

    // What the export refuses, with the message; a device address carries no capacity to check.
    private void checkArguments(long nstripes, long byteCount, long base, long suspect, long culprit, long healId) {
        if (nstripes < 0 || byteCount < 0) {
            throw new IllegalArgumentException("negative count");
        }
        if (healId != 0 && shardCount > 255) {
            throw new IllegalArgumentException("heal ids are bytes: at most 255 shards");
        }
        if (nstripes > 0 && (base == 0 || suspect == 0 || culprit == 0)) {
            throw new NullPointerException("null device address");
        }
    }

    /** Parity shards of the codec. */
    public int parityShardCount() {
        return parityCount;
    }

    private long handle() {
        if (rs == 0) {
            throw new IllegalStateException("EcxCorruptLocate is closed");
        }
        return rs;
    }

    /** Releases this wrapper's reference to the shared native codec; idempotent (see EcxPartialSums). */
    public synchronized void close() {
        if (rs == 0) {
            return;
        }
        long h = rs;
        rs = 0;
        EcxNative.rsDestroy(h);
    }
}
