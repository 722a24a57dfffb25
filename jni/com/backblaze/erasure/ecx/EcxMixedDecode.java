package com.backblaze.erasure.ecx;

/**
 * ReedSolomon.decodeMissing (ReedSolomon.java:189-286) over many device-resident stripes that
 * miss different shards, in one launch, on libecx.so: the erasure patterns of a batch are
 * compiled once into a pattern set, and each stripe names its pattern with one byte of a device
 * array.  A stripe whose pattern misses nothing, or whose id names no pattern, is left untouched.
 * The set must stay open until the work enqueued with it has finished; the first decode on a
 * device must run outside stream capture.
 */
public final class EcxMixedDecode {
    private long rs;   // 0 once closed
    private long set;  // 0 once closed
    private final int shardCount;

    /**
     * The codec of ReedSolomon.create(dataShards, parityShards) and the patterns
     * {@code shardPresent[p]} (1..256 of them, each of dataShards + parityShards flags, at most
     * 8 of them false and at least dataShards true).
     */
    public EcxMixedDecode(int dataShards, int parityShards, boolean[][] shardPresent) {
        this.shardCount = dataShards + parityShards;
        if (shardPresent == null) {
            throw new NullPointerException("shardPresent");
        }
        byte[] flags = new byte[shardPresent.length * shardCount];
        for (int p = 0; p < shardPresent.length; ++p) {
            if (shardPresent[p] == null || shardPresent[p].length != shardCount) {
                throw new IllegalArgumentException("pattern " + p + " needs " + shardCount + " flags");
            }
            System.arraycopy(Ecx.flags(shardPresent[p]), 0, flags, p * shardCount, shardCount);
        }
        this.rs = Ecx.createReedSolomon(dataShards, parityShards);
        long[] out = new long[1];
        int st = EcxNative.rsPatternSetCreate(rs, flags, shardPresent.length, out);
        if (st < 0) {
            close();
            Ecx.check(st);
        }
        this.set = out[0];
    }

    /**
     * The distinct rows of {@code shardPresent} (one row per stripe) in order of first appearance,
     * and into {@code ids} (one byte per stripe) the index of each stripe's row among them: the
     * patterns to build an EcxMixedDecode from and the ids to copy to the device.
     */
    public static boolean[][] indexPatterns(boolean[][] shardPresent, byte[] ids) {
        int n = shardPresent.length == 0 ? 1 : shardPresent[0].length;
        byte[] present = new byte[shardPresent.length * n];
        for (int s = 0; s < shardPresent.length; ++s) {
            if (shardPresent[s].length != n) {
                throw new IllegalArgumentException("stripe " + s + " needs " + n + " flags");
            }
            System.arraycopy(Ecx.flags(shardPresent[s]), 0, present, s * n, n);
        }
        byte[] patterns = new byte[256 * n];
        int[] count = new int[1];
        Ecx.check(EcxNative.rsIndexPatterns(n, present, shardPresent.length, patterns, 256, count, ids));
        boolean[][] out = new boolean[count[0]][n];
        for (int p = 0; p < count[0]; ++p) {
            for (int i = 0; i < n; ++i) {
                out[p][i] = patterns[p * n + i] != 0;
            }
        }
        return out;
    }

    /**
     * decodeMissing of stripe s (shard i at base + s * stripeStride + i * shardStride, device
     * memory) with pattern patternOfStripe[s] (a device byte array of nstripes) over bytes
     * [offset, offset + byteCount), in place.  Only enqueues on {@code stream} (0 = the default).
     */
    public void decodeMissingBatch(long patternOfStripe, long base, long stripeStride, long shardStride, long nstripes,
                                   long offset, long byteCount, long stream) {
        Ecx.check(EcxNative.rsDecodeMissingBatchMixed(handle(), patternOfStripe, base, stripeStride, shardStride,
                nstripes, offset, byteCount, stream));
    }

    /**
     * decodeMissingBatch over nstripes device-resident stripes in the blocked layout
     * (EcxBlockedStripes; body [nstripes][full][n][block], then tails [nstripes][n][tail]), in
     * place: stripe s is decoded with pattern patternOfStripe[s] (a device byte array of
     * nstripes).  blockBytes 0 = the recommended block.  Only enqueues on {@code stream}.
     */
    public void decodeMissingBlockedBatch(long patternOfStripe, long base, long nstripes, long byteCount,
                                          long blockBytes, long stream) {
        Ecx.check(EcxNative.rsDecodeMissingBlockedBatchMixed(handle(), patternOfStripe, base, nstripes, byteCount,
                blockBytes, stream));
    }

    /**
     * decodeMissingBatch over HOST-memory stripes at raw addresses, synchronous.  Package-private:
     * a raw host address carries no capacity to check (no ByteBuffer form yet; INTEGRATION.md).
     */
    void decodeMissingBatchHost(long patternOfStripe, long base, long stripeStride, long shardStride, long nstripes,
                                long offset, long byteCount) {
        Ecx.check(EcxNative.rsDecodeMissingMixedBatchHost(handle(), patternOfStripe, base, stripeStride, shardStride,
                nstripes, offset, byteCount));
    }

    /** decodeMissingBlockedBatch over HOST-memory stripes at raw addresses, synchronous; package-private likewise. */
    void decodeMissingBlockedBatchHost(long patternOfStripe, long base, long nstripes, long byteCount,
                                       long blockBytes) {
        Ecx.check(EcxNative.rsDecodeMissingBlockedMixedBatchHost(handle(), patternOfStripe, base, nstripes, byteCount,
                blockBytes));
    }

    /**
     * One hop of the pipelined repair chain (ReedSolomon.decodeMissingSingle,
     * ReedSolomon.java:288-333, for every missing shard) with a pattern and a helper shard index per
     * stripe: for stripe s, shard shardOfStripe[s] -- read at
     * in + s * inStripeStride + shardOfStripe[s] * inShardStride; inShardStride 0 = this helper's own
     * shards back to back -- adds its contribution to every shard that pattern patternOfStripe[s]
     * misses: acc + s * accStripeStride + o * accRowStride is assigned when isFirst, XOR-accumulated
     * otherwise, for o over the pattern's missing shards in ascending order.  Both arrays are device
     * byte arrays of nstripes.  Rows past a pattern's missing count, and stripes whose id names no
     * pattern, whose pattern misses nothing or whose shard byte is no shard, are left untouched.
     * in and acc must not overlap.  Only enqueues on {@code stream}; the first hop on a device must
     * run outside stream capture.
     */
    public void decodePartialBatch(long patternOfStripe, long shardOfStripe, long in, long inStripeStride,
                                   long inShardStride, long acc, long accStripeStride, long accRowStride,
                                   long nstripes, long byteCount, boolean isFirst, long stream) {
        Ecx.check(EcxNative.rsDecodePartialBatchMixed(handle(), patternOfStripe, shardOfStripe, in, inStripeStride,
                inShardStride, acc, accStripeStride, accRowStride, nstripes, byteCount, isFirst ? 1 : 0, stream));
    }

    /** {patterns, shards per stripe, most shards any pattern misses}. */
    public int[] info() {
        int[] n = new int[1], shards = new int[1], missing = new int[1];
        Ecx.check(EcxNative.rsPatternSetInfo(handle(), n, shards, missing));
        return new int[] {n[0], shards[0], missing[0]};
    }

    private long handle() {
        if (set == 0) {
            throw new IllegalStateException("EcxMixedDecode is closed");
        }
        return set;
    }

    /** Frees the pattern set and releases this wrapper's codec reference; idempotent (see EcxPartialSums). */
    public synchronized void close() {
        long s = set, h = rs;
        set = 0;
        rs = 0;
        if (s != 0) {
            EcxNative.rsPatternSetDestroy(s);
        }
        if (h != 0) {
            EcxNative.rsDestroy(h);
        }
    }
}
