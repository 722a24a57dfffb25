package com.backblaze.erasure.ecx;

/**
 * The scrub of a store that keeps Clay stripes: whether each of many DEVICE-resident stripes of
 * Clay(dataUnits, parityUnits) -- shortened by virtualUnits zero data nodes -- is still a codeword,
 * in one read-only launch on libecx.so (ecx_clay_is_parity_correct_batch).  The reference has no
 * counterpart: its only route is to re-encode the parity nodes and compare.  It is a codeword test:
 * a failing stripe's verdict does not say which node is corrupt.
 * The stripes lie as ClayCodeErasureDecodingStep.performCoding's inputs do: real slot
 * z * (dataUnits + parityUnits) + node of stripe s at base + s * stripeStride + slot * subStride.
 * A device address carries no capacity to check, so the call that takes addresses is
 * package-private: the classes of this package that own device memory hand it theirs.
 */
public final class EcxClayParityCheck {
    private long clay;  // 0 once closed; holds the shared codec, and with it the proved check program
    private final int dataUnits;
    private final int parityUnits;
    private final int virtualUnits;
    private final int[] geometry = new int[4];  // q, t, alpha, real nodes

    /** The geometry of ClayCodeErasureDecodingStep(dataUnits + virtualUnits, parityUnits); at most 8 parity units. */
    public EcxClayParityCheck(int dataUnits, int parityUnits, int virtualUnits) {
        if (dataUnits < 1 || parityUnits < 1 || virtualUnits < 0) {
            throw new IllegalArgumentException("unit counts");
        }
        if (parityUnits > 8) {
            throw new IllegalArgumentException("the Clay parity check takes at most 8 parity units");
        }
        long[] h = new long[1];
        Ecx.check(EcxNative.clayCreateShortened(dataUnits, parityUnits, virtualUnits, new int[0], 0, h));
        this.clay = h[0];
        this.dataUnits = dataUnits;
        this.parityUnits = parityUnits;
        this.virtualUnits = virtualUnits;
        int[] q = new int[1], t = new int[1], alpha = new int[1];
        Ecx.check(EcxNative.clayGeometry(clay, q, t, alpha));
        geometry[0] = q[0];
        geometry[1] = t[0];
        geometry[2] = alpha[0];
        geometry[3] = dataUnits + parityUnits;
    }

    /** {q, t, alpha, real nodes}: a stripe holds alpha * nodes sub-chunks. */
    public int[] geometry() {
        return geometry.clone();
    }

    /** Sub-chunks of one stripe: the slots the layout addresses. */
    public long slotsPerStripe() {
        return (long) geometry[2] * geometry[3];
    }

    /**
     * ecx_clay_is_parity_correct_batch: {@code verdict} (device bytes, nstripes) receives 1 for each
     * stripe that is a codeword over bytes [0, bufSize) of every sub-chunk, else 0.  Only enqueues on
     * {@code stream} (0 = the default); the first call of a geometry on a device must run outside
     * stream capture.
     */
    void isParityCorrectBatch(long base, long stripeStride, long subStride, long nstripes, long bufSize, long verdict,
                              long stream) {
        handle();
        if (nstripes < 0 || bufSize < 0) {
            throw new IllegalArgumentException("negative count");
        }
        if (nstripes > 0 && (base == 0 || verdict == 0)) {
            throw new NullPointerException("null device address");
        }
        if (nstripes > 0 && (stripeStride < 0 || subStride < 0)) {
            throw new IllegalArgumentException("negative stride");
        }
        Ecx.check(EcxNative.clayIsParityCorrectBatch(dataUnits, parityUnits, virtualUnits, base, stripeStride,
                subStride, nstripes, bufSize, verdict, stream));
    }

    private long handle() {
        if (clay == 0) {
            throw new IllegalStateException("EcxClayParityCheck is closed");
        }
        return clay;
    }

    /** Releases this wrapper's reference to the shared native codec; idempotent (see EcxPartialSums). */
    public synchronized void close() {
        if (clay == 0) {
            return;
        }
        long h = clay;
        clay = 0;
        EcxNative.clayDestroy(h);
    }
}
