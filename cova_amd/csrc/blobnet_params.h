// The BlobNet architecture and its parameter blob, stated once for the forward (blobnet.hip, blobnet_mfma.hip) and the trainer
// (train.hip): a trainer's blob must load into the forward.  No HIP types here.  The Python side of the same layout is
// cova_amd/weights.py.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

constexpr int BN_T = 4;       // timestep the network is built for (utils/train-blobnet.py:58)
constexpr int BN_LEVELS = 4;  // encoder levels / decoder blocks
constexpr int BN_ENC_C[BN_LEVELS + 1] = {3, 16, 32, 64, 128};
constexpr int BN_DEC_CI[BN_LEVELS] = {128, 128, 64, 32};
constexpr int BN_DEC_CO[BN_LEVELS] = {64, 32, 16, 16};
constexpr size_t BN_N_PARAMS = 320305;

// A CVHW blob: this 64-byte header (a reader checks the first 13 words), then the BN_N_PARAMS fp32 parameters.
constexpr size_t BN_HEADER_BYTES = 64;
// Words: "CVHW", version, timestep, the encoder's channels, the decoder blocks' output channels, the parameter count, zeros.
constexpr uint32_t BN_HEADER[16] = {0x57485643, 1, BN_T, BN_ENC_C[0], BN_ENC_C[1], BN_ENC_C[2], BN_ENC_C[3], BN_ENC_C[4],
                                    BN_DEC_CO[0], BN_DEC_CO[1], BN_DEC_CO[2], BN_DEC_CO[3], (uint32_t)BN_N_PARAMS, 0, 0, 0};
constexpr size_t BN_BLOB_BYTES = BN_HEADER_BYTES + BN_N_PARAMS * sizeof(float);

// Offsets of every tensor in the flat parameters, in floats.  Encoder level i: 3x3 conv kernel [3][3][ci][co], bias, BN gamma /
// beta / moving mean / moving variance, the temporal MLP's w1 and w2 [T][T].  Decoder block j: 4x4 transposed-conv kernel, bias
// and -- blocks 0 .. 2 -- BN gamma / beta / mean / variance (block 3's stay 0).  Then the final 1x1 kernel [16] and bias.
struct BnEncOff { size_t k, b, gamma, beta, mean, var, w1, w2; };
struct BnDecOff { size_t k, b, gamma, beta, mean, var; };
struct BnLayout {
    BnEncOff enc[BN_LEVELS];
    BnDecOff dec[BN_LEVELS];
    size_t fk, fb, end;
};
constexpr BnLayout bn_layout() {
    BnLayout l{};
    size_t off = 0;
    auto take = [&off](size_t n) { const size_t at = off; off += n; return at; };
    for (int i = 0; i < BN_LEVELS; i++) {
        const size_t ci = BN_ENC_C[i], co = BN_ENC_C[i + 1];
        l.enc[i] = {take(9 * ci * co), take(co), take(co), take(co), take(co), take(co), take(BN_T * BN_T), take(BN_T * BN_T)};
    }
    for (int j = 0; j < BN_LEVELS; j++) {
        const size_t ci = BN_DEC_CI[j], co = BN_DEC_CO[j];
        l.dec[j].k = take(16 * ci * co);
        l.dec[j].b = take(co);
        if (j < BN_LEVELS - 1) {
            l.dec[j].gamma = take(co);
            l.dec[j].beta = take(co);
            l.dec[j].mean = take(co);
            l.dec[j].var = take(co);
        }
    }
    l.fk = take(16);
    l.fb = take(1);
    l.end = off;
    return l;
}
constexpr BnLayout BN_LAYOUT = bn_layout();
static_assert(BN_LAYOUT.end == BN_N_PARAMS, "the layout and the parameter count disagree");

// The parameters of a CVHW blob of this architecture (behind the header), or null: a header word or the size is off.
inline const float *bn_check_blob(const void *blob, size_t bytes) {
    if (!blob || bytes != BN_BLOB_BYTES || std::memcmp(blob, BN_HEADER, 13 * sizeof(uint32_t)) != 0) return nullptr;
    return reinterpret_cast<const float *>(static_cast<const uint8_t *>(blob) + BN_HEADER_BYTES);
}
