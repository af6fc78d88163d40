// ref_rules.h -- the reference's arithmetic rules, each stated ONCE; included by rpcc_hip.hip right after rpcc_device.h.
//
// Bit-exact parity (DESIGN.md sections 2 and 3) holds because every rule below is one fixed sequence of operations.  The
// encoder and the decoder, the byte-label kernels and the uint16 ones (wide_kernels.h) all call these functions: an edit
// here reaches every user at once, and no kernel carries a copy of its own.  A caller keeps what is its own -- where its
// operands come from (LDS or memory), the integer type of its totals -- and converts at the call.
#pragma once

// a10  intra_predict (cpp_modules.cpp:248-285): the range a label's model row (a, b, c, d) predicts along the ray (tx, ty, tz).
__device__ __forceinline__ float intra_pred(float a, float b, float c, float d, float tx, float ty, float tz) {
    float pr;
    if (a + b + c == 0.0f) pr = d;                      // a point model's row (0, 0, 0, mean): cpp_modules.cpp:271-272
    else pr = -d / (a * tx + b * ty + c * tz);          // a plane: :275-277
    return pr;
}

// a8  one (frame, label) row of the point model (cpp_modules.cpp:471-518, segment_utils.py:183-185): the ground plane for label 0,
// zeros for label 1 (empty pixels), else (0, 0, 0, mean range) -- the default NaN of x86's 0.0 / 0 for a label without pixels.
// The mean's sum is `fixed_sum` units of 2^-28 m (exact, below 2^53: DESIGN.md "point model") unless the frame's flag says that some
// range fell outside the fixed-point window [2^-5, 2^8): then the reference's own sequential double accumulation in row-major
// order (:514), one thread per label, rare.  model [B,K,4], ground [B,4], flags [B,4], seg and ri [B,P]: the batch's; b, k: the row.
template <class L, class N>
__device__ __forceinline__ void point_model_row(float *model, const double *ground, const int32_t *flags, const L *seg, const float *ri,
                                                int P, int K, int b, int k, long long fixed_sum, N total) {
    float *row = model + ((int64_t)b * K + k) * 4;
    if (k == 0) {
        row[0] = (float)ground[4 * b]; row[1] = (float)ground[4 * b + 1]; row[2] = (float)ground[4 * b + 2]; row[3] = (float)ground[4 * b + 3];
    } else if (k == 1) {
        row[0] = row[1] = row[2] = row[3] = 0.0f;
    } else {
        double s;
        if (flags[4 * b]) {
            s = 0.0;
            const L *sg = seg + (int64_t)b * P;
            const float *rr = ri + (int64_t)b * P;
            for (int p = 0; p < P; p++)
                if (sg[p] == k) s += (double)rr[p];
        } else {
            s = (double)fixed_sum * (1.0 / 268435456.0);
        }
        row[0] = row[1] = row[2] = 0.0f;
        row[3] = total == 0 ? rpcc::u2f(0xFFC00000u) : (float)(s / (double)total);
    }
}

// a13  salience level of label k from its pixel and key-point totals (cpp_modules.cpp:388-403): label 0 -> ground_level, label 1 and
// labels of fewer than 30 pixels -> the last level, else the first level whose level_kp_num the key points reach (level 0 if none).
struct SalienceParams {
    int level_kp_num[8];
    float level_acc[8];
    int levels, ground_level;
};
__device__ __forceinline__ int salience_level(int k, int pixels, int keypoints, const SalienceParams &sp) {
    int lv = 0;
    if (k == 0) lv = sp.ground_level;
    else if (k == 1) lv = sp.levels - 1;
    else if (pixels < 30) lv = sp.levels - 1;
    else
        for (int l = 0; l < sp.levels; l++)
            if (keypoints >= sp.level_kp_num[l]) { lv = l; break; }
    return lv;
}

// a11 / a13  quantisation of a residual (cpp_modules.cpp:315; step: the uniform accuracy or the label's, :404,419).  The caller
// stores the integer as int16 (astype(np.int16): two's-complement truncation) or int32.
// The conversion rule: a rounded quotient that is NaN or outside [-2^31, 2^31) gives INT_MIN -- what the reference's x86 binary returns
// (cvttss2si's "integer indefinite"; int16: 0) for a C expression that is undefined there.  The device's own conversion saturates
// (+overflow -> INT_MAX, int16 -1) and turns NaN into 0, so the rule is stated, not left to the instruction; NaN fails the comparison,
// and -2^31 converts to INT_MIN either way.  Reached by far returns sharing a cluster, by infinite or NaN predictions (a horizontal beam
// against a horizontal plane row) and by a zero step: DESIGN.md section 3, tests/value_cases.py.
// (NaN VALUES elsewhere -- predictions, reconstructions -- are held to the oracle by their places only; observed, not asserted: the 0 / 0 and
// inf * 0 NaNs of tests/value_cases.py's scene B carry x86's default pattern 0xFFC00000 on gfx950 too.)
__device__ __forceinline__ int quantise(float res, float step) {
    const float r = roundf(res / step);
    return fabsf(r) < 2147483648.0f ? (int)r : INT_MIN;
}

// f3  dequantize_residual (compress_utils.py:114-132).  The step: one double (uniform: levels == 0, salience is not read and may be NULL)
// or that of the label's level salience[i]; the residual: int16 * python float -> float64 -> stored into a float32 array.
// (A level beyond the configured ones -- a corrupt stream; tools/decompress.py rejects it -- is clamped, never read past acc[].)
struct DecodeSteps {
    double acc[8];  // acc[level]; uniform: acc[0]
    int levels;     // 0 = uniform
};
__device__ __forceinline__ double dequant_step(const DecodeSteps &steps, const uint8_t *salience, int64_t i) {
    return steps.levels ? steps.acc[min((int)salience[i], steps.levels - 1)] : steps.acc[0];
}
__device__ __forceinline__ float dequant(int16_t q, double step) { return (float)((double)q * step); }

// a3  a pixel's point as the label-ordered lists hold it: range * ray, and the range (transformer.py:94-101)
__device__ __forceinline__ float4 label_point(float r, float tx, float ty, float tz) { return make_float4(r * tx, r * ty, r * tz, r); }
