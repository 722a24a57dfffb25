package com.backblaze.erasure.ecx;

/**
 * The step between the scrub and the repair: which shard is corrupt in each stripe that fails
 * ReedSolomon.isParityCorrect (ReedSolomon.java:129-178), over many DEVICE-resident stripes at
 * once, on libecx.so.  The reference has no counterpart.  Read-only on the stripes; the answers are
 * device arrays, so an EcxMixedDecode built from the shards' single-loss patterns in shard order
 * (pattern j: only shard j missing) heals the batch from {@code healId} on the same stream with no
 * host round trip.  With two parity shards, two corrupt shards at the same byte position can
 * imitate a third one; with three or more a code of distance m + 1 tells two errors from one, and
 * with four or more locateCorrupt2 names both (doubleLossPatterns heals them).
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

    /** The place of the pair {i, j}, i &lt; j, among the pairs of this code's shards in lexicographic order. */
    public int pairIndex(int i, int j) {
        if (i < 0 || i >= j || j >= shardCount) {
            throw new IllegalArgumentException("a pair is 0 <= i < j < shards");
        }
        return i * (2 * shardCount - i - 1) / 2 + (j - i - 1);
    }

    /**
     * The single-loss patterns in shard order, then the pair-loss patterns in pair order (pattern
     * shards + pairIndex(i, j): shards i and j missing): what to build the EcxMixedDecode from that
     * heals the batch from locateCorrupt2's {@code healId}.  At most 22 shards (256 patterns).
     */
    public boolean[][] doubleLossPatterns() {
        int pairs = shardCount * (shardCount - 1) / 2;
        if (shardCount + pairs > 255) {
            throw new IllegalArgumentException("heal ids are bytes: at most 22 shards");
        }
        boolean[][] p = new boolean[shardCount + pairs][];
        System.arraycopy(singleLossPatterns(), 0, p, 0, shardCount);
        for (int i = 0; i < shardCount; ++i) {
            for (int j = i + 1; j < shardCount; ++j) {
                boolean[] row = new boolean[shardCount];
                java.util.Arrays.fill(row, true);
                row[i] = false;
                row[j] = false;
                p[shardCount + pairIndex(i, j)] = row;
            }
        }
        return p;
    }

    /**
     * ecx_rs_locate_corrupt2_batch: locateCorrupt's arguments, naming up to two corrupt shards.
     * {@code suspect} (device bytes, nstripes * (shards + pairs)) receives the single suspects, then 1
     * at shards + pairIndex(i, j) where replacing shards i and j together can make the stripe pass;
     * {@code culprit} (device ints, 2 * nstripes) (-1, -1) for a clean stripe, (j, -1) for one
     * corrupt shard, (i, j) for two, (-2, -2) otherwise; {@code healId} (device bytes, nstripes; 0 =
     * not wanted) j, shards + pairIndex(i, j) or 255.  Codes with 4 to 8 parity shards and at most 64
     * shards.  Three corrupt shards can imitate a pair of other shards.
     */
    public void locateCorrupt2(long base, long stripeStride, long shardStride, long nstripes, long firstByte,
                               long byteCount, long suspect, long culprit, long healId, long stream) {
        checkArguments2(nstripes, byteCount, base, suspect, culprit, healId);
        if (stripeStride < 0 || shardStride < 0 || firstByte < 0) {
            throw new IllegalArgumentException("negative stride or first byte");
        }
        Ecx.check(EcxNative.rsLocateCorrupt2Batch(handle(), base, stripeStride, shardStride, nstripes, firstByte,
                byteCount, suspect, culprit, healId, stream));
    }

    /**
     * locateCorrupt2 over nstripes device-resident stripes in the blocked layout
     * (ecx_rs_locate_corrupt2_blocked_batch; locateCorruptBlocked's arguments).  {@code healId} feeds
     * EcxMixedDecode.decodeMissingBlockedBatch.
     */
    public void locateCorrupt2Blocked(long base, long nstripes, long byteCount, long blockBytes, long suspect,
                                      long culprit, long healId, long stream) {
        checkArguments2(nstripes, byteCount, base, suspect, culprit, healId);
        if (blockBytes < 0) {
            throw new IllegalArgumentException("negative block size");
        }
        Ecx.check(EcxNative.rsLocateCorrupt2BlockedBatch(handle(), base, nstripes, byteCount, blockBytes, suspect,
                culprit, healId, stream));
    }

    // What the two-shard exports refuse, in their order and with the message.
    private void checkArguments2(long nstripes, long byteCount, long base, long suspect, long culprit, long healId) {
        if (nstripes < 0 || byteCount < 0) {
            throw new IllegalArgumentException("negative count");
        }
        if (parityCount < 4) {
            throw new IllegalArgumentException("locating two shards takes codes with 4 to 8 parity shards");
        }
        if (shardCount > 64) {
            throw new IllegalArgumentException("locating two shards takes at most 64 shards");
        }
        if (healId != 0 && shardCount > 22) {
            throw new IllegalArgumentException("heal ids are bytes: at most 22 shards");
        }
        if (nstripes > 0 && (base == 0 || suspect == 0 || culprit == 0)) {
            throw new NullPointerException("null device address");
        }
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
