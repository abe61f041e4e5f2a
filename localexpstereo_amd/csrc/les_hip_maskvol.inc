// les_hip_maskvol.inc -- part of the single translation unit les_hip.hip (included there; not compiled on its own): the launch of the
// nearest-valid row fill of a cost volume (csrc/les_maskvol.h holds the rule and the kernel) -- les_hip_fill_invalid.
extern "C" {

int les_hip_fill_invalid(float* d_vol, int D, int H, int W, int mode, int d0, const uint8_t* d_validI, const uint8_t* d_validJ, float fill, int device,
                         void* stream)
{
    if (!d_vol) return fail(LES_HIP_ERR_ARG, "les_hip_fill_invalid: null volume");
    if (mode < 0 || mode > 1) return fail(LES_HIP_ERR_ARG, "les_hip_fill_invalid: mode %d (0 or 1)", mode);
    if (D <= 0 || H <= 0 || W <= 0) return fail(LES_HIP_ERR_ARG, "les_hip_fill_invalid: bad volume size %d x %d x %d", D, H, W);
    if (!std::isfinite(fill)) return fail(LES_HIP_ERR_ARG, "les_hip_fill_invalid: fill %g (finite)", (double)fill);
    if (W > les::kMvMaxW) return fail(LES_HIP_ERR_UNSUPPORTED, "les_hip_fill_invalid: rows of %d entries (at most %d)", W, les::kMvMaxW);
    if (H > 65535) return fail(LES_HIP_ERR_UNSUPPORTED, "les_hip_fill_invalid: %d rows (at most 65535)", H);
    const long long chunks = ((long long)D + les::kMvDC - 1) / les::kMvDC;
    if (chunks > 65535) return fail(LES_HIP_ERR_UNSUPPORTED, "les_hip_fill_invalid: %d slices (at most %d)", D, 65535 * les::kMvDC);
    if ((long long)D * H * W >= (1ll << 32))                 // (H <= 65535 and W <= kMvMaxW: the product fits 64 bits)
        return fail(LES_HIP_ERR_UNSUPPORTED, "les_hip_fill_invalid: a volume of %d x %d x %d has 2^32 entries or more", D, H, W);
    HIPCHECK(hipSetDevice(device));
    uint32_t fill_bits;
    memcpy(&fill_bits, &fill, 4);
    uint32_t* vol = reinterpret_cast<uint32_t*>(d_vol);
    const dim3 grid((unsigned)chunks, (unsigned)H), block(les::kMvNT);
    if (((uintptr_t)d_vol & 15) == 0 && W % 4 == 0)          // every row starts 16-byte aligned
        hipLaunchKernelGGL(les::les_fill_invalid_kernel<true>, grid, block, 0, (hipStream_t)stream, vol, D, H, W, mode, d0, d_validI, d_validJ, fill_bits);
    else
        hipLaunchKernelGGL(les::les_fill_invalid_kernel<false>, grid, block, 0, (hipStream_t)stream, vol, D, H, W, mode, d0, d_validI, d_validJ, fill_bits);
    HIPCHECK(hipGetLastError());
    return LES_HIP_OK;
}

}  // extern "C"
