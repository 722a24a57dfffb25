package com.backblaze.erasure.ecx;

/**
 * ClayCodeErasureDecodingStep.performCoding (ClayCodeErasureDecodingStep.java:53-107) over many
 * stripes that lost different nodes, in one launch, on libecx.so: the erased-node lists of a
 * batch are compiled once into a pattern set, and each stripe names its list with one byte.
 * Stripe s holds n*alpha sub-chunks (slot z*n + node) and receives the |E|*alpha sub-chunks of its
 * own list (slot z*|E| + j).  A stripe whose list is empty, or whose id names no list, is left
 * untouched by the device form and gets zeros from the host form.  Single-node lists of the
 * geometries with 256 rows per node (Clay(12,4), the shortened Clay(10,4)) form a generated set:
 * its kernel is generated and compiled on the first repair, and it takes sub-chunk sizes that are
 * multiples of 4096 in 16-byte-aligned layouts only.  Lists of more than 64 rows that erase
 * several nodes are refused: repair those with EcxClayCodeErasureDecodingStep.
 * The set must stay open until the work enqueued with it has finished; the first repair on a
 * device must run outside stream capture.
 */
public final class EcxClayMixedRepair {
    private long set;  // 0 once closed

    /** The lists {@code erasedIndexes[p]} (1..256 of them) of Clay(dataUnits, parityUnits), shortened by virtualUnits. */
    public EcxClayMixedRepair(int dataUnits, int parityUnits, int virtualUnits, int[][] erasedIndexes) {
        if (erasedIndexes == null) {
            throw new NullPointerException("erasedIndexes");
        }
        int total = 0;
        int[] counts = new int[erasedIndexes.length];
        for (int p = 0; p < erasedIndexes.length; ++p) {
            if (erasedIndexes[p] == null) {
                throw new NullPointerException("erasedIndexes[" + p + "]");
            }
            counts[p] = erasedIndexes[p].length;
            total += counts[p];
        }
        int[] flat = new int[total];
        for (int p = 0, at = 0; p < erasedIndexes.length; at += counts[p], ++p) {
            System.arraycopy(erasedIndexes[p], 0, flat, at, counts[p]);
        }
        long[] out = new long[1];
        Ecx.check(EcxNative.clayPatternSetCreate(dataUnits, parityUnits, virtualUnits, flat, counts,
                erasedIndexes.length, out));
        this.set = out[0];
    }

    /**
     * performCoding of stripe s (sub-chunk i at in + s * inStripeStride + i * inSubStride, device
     * memory) with list patternOfStripe[s] (a device byte array of nstripes) into
     * out + s * outStripeStride + o * outSubStride, bufSize bytes per sub-chunk.  in and out must
     * not overlap.  Only enqueues on {@code stream} (0 = the default).
     */
    public void performCodingBatch(long patternOfStripe, long in, long inStripeStride, long inSubStride, long out,
                                   long outStripeStride, long outSubStride, long nstripes, long bufSize, long stream) {
        Ecx.check(EcxNative.clayPerformCodingBatchMixed(handle(), patternOfStripe, in, inStripeStride, inSubStride, out,
                outStripeStride, outSubStride, nstripes, bufSize, stream));
    }

    /**
     * One hop of the pipelined repair chain (ClayCoordinator.kt:265-319, ClayCodeNode.kt:165-233)
     * with a list and a helper node per stripe: stripe s adds node nodeOfStripe[s]'s share of list
     * patternOfStripe[s]'s repair (both device byte arrays of nstripes) to the rows at
     * acc + s * accStripeStride + r * accSubStride, or assigns them when isFirst.  Plane z of the
     * node lies at in + s * inStripeStride + nodeOfStripe[s] * inNodeStride + z * inSubStride
     * (inNodeStride 0: this helper's own sub-chunks back to back).  in and acc must not overlap.
     * Only enqueues on {@code stream} (0 = the default).
     */
    public void partialBatch(long patternOfStripe, long nodeOfStripe, long in, long inStripeStride, long inNodeStride,
                             long inSubStride, long acc, long accStripeStride, long accSubStride, long nstripes,
                             long bufSize, boolean isFirst, long stream) {
        Ecx.check(EcxNative.clayPartialBatchMixed(handle(), patternOfStripe, nodeOfStripe, in, inStripeStride,
                inNodeStride, inSubStride, acc, accStripeStride, accSubStride, nstripes, bufSize, isFirst ? 1 : 0,
                stream));
    }

    /**
     * performCodingBatch over HOST-memory stripes at raw addresses, synchronous: output slots
     * 0 .. maxErased*alpha - 1 come back for every stripe, and what a stripe's own list does not
     * write comes back as zeros.  Package-private: a raw host address carries no capacity to check
     * (no ByteBuffer form yet; INTEGRATION.md).
     */
    void performCodingBatchHost(long patternOfStripe, long in, long inStripeStride, long inSubStride, long out,
                                long outStripeStride, long outSubStride, long nstripes, long bufSize) {
        Ecx.check(EcxNative.clayPerformCodingMixedBatchHost(handle(), patternOfStripe, in, inStripeStride, inSubStride,
                out, outStripeStride, outSubStride, nstripes, bufSize));
    }

    /** {lists, nodes per stripe, alpha, most nodes any list erases}. */
    public int[] info() {
        int[] n = new int[1], nodes = new int[1], alpha = new int[1], erased = new int[1];
        Ecx.check(EcxNative.clayPatternSetInfo(handle(), n, nodes, alpha, erased));
        return new int[] {n[0], nodes[0], alpha[0], erased[0]};
    }

    private long handle() {
        if (set == 0) {
            throw new IllegalStateException("EcxClayMixedRepair is closed");
        }
        return set;
    }

    /** Frees the pattern set and the codec references it holds; idempotent (see EcxPartialSums). */
    public synchronized void close() {
        long s = set;
        set = 0;
        if (s != 0) {
            EcxNative.clayPatternSetDestroy(s);
        }
    }
}
