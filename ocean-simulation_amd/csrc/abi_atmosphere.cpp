// C-ABI layer of liboceanhip.so, the atmosphere (ocean.h): ocean_atmosphere, ocean_sky_update, ocean_atmosphere_read,
// ocean_atmosphere_lut and ocean_sun_color.  The context owns the three tables (ocean_ctx::atm); the camera's
// OCEAN_CAMERA_SKY_LUT mode reads the third (abi_consumers.cpp).  Every argument that can be judged without the
// context is judged before the context is looked at, so a host learns of a bad argument whatever its context is.
#include <cmath>

#include "abi_internal.h"

namespace {

constexpr int kDefaultDims[6] = {64, 256, 64, 64, 256, 128};  // AtmosphereController.cs:12-19
const char* const kDimNames[6] = {"transmittance_width", "transmittance_height", "multiscatter_width",
                                  "multiscatter_height", "skyview_width",       "skyview_height"};

// ocean.h, "the sun": n = sun / |sun| in fp32, len = sqrtf((x * x + y * y) + z * z), three divisions.
int normalise_sun(const float* sun, float n[3]) {
    if (!sun) return fail(OCEAN_E_INVALID_ARG, "null sun");
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(sun[k])) return fail(OCEAN_E_INVALID_ARG, "sun[" + std::to_string(k) + "] is not finite");
    const float len = std::sqrt((sun[0] * sun[0] + sun[1] * sun[1]) + sun[2] * sun[2]);
    if (!(len > 0.0f) || !std::isfinite(len)) return fail(OCEAN_E_INVALID_ARG, "sun must have a finite length > 0");
    for (int k = 0; k < 3; ++k) n[k] = sun[k] / len;
    return OCEAN_OK;
}

int check_which(int which) {
    if (which != OCEAN_LUT_TRANSMITTANCE && which != OCEAN_LUT_MULTISCATTER && which != OCEAN_LUT_SKYVIEW)
        return fail(OCEAN_E_INVALID_ARG, "unknown which (OCEAN_LUT_*)");
    return OCEAN_OK;
}

int check_ready(const ocean_ctx* ctx, const char* entry) {
    if (!ctx->atm.ready) return fail(OCEAN_E_STATE, std::string("ocean_atmosphere must precede ") + entry);
    return OCEAN_OK;
}

}  // namespace

extern "C" {

int ocean_atmosphere(ocean_ctx* ctx, const float* params, int transmittance_width, int transmittance_height,
                     int multiscatter_width, int multiscatter_height, int skyview_width, int skyview_height) {
    if (!params) return fail(OCEAN_E_INVALID_ARG, "null params");
    for (int k = 0; k < OCEAN_ATMOSPHERE_FLOATS; ++k)
        if (!std::isfinite(params[k])) return fail(OCEAN_E_INVALID_ARG, "params[" + std::to_string(k) + "] is not finite");
    if (!(params[0] > 0.0f)) return fail(OCEAN_E_INVALID_ARG, "planetRadius (params[0]) must be > 0");
    if (!(params[1] > params[0])) return fail(OCEAN_E_INVALID_ARG, "atmosphereRadius (params[1]) must be > planetRadius");
    if (!(params[8] > 0.0f) || !(params[15] > 0.0f))
        return fail(OCEAN_E_INVALID_ARG, "the Rayleigh and Mie scale height (params[8], params[15]) must be > 0");
    for (int k = 27; k < OCEAN_ATMOSPHERE_FLOATS; ++k)
        if (params[k] != 0.0f) return fail(OCEAN_E_INVALID_ARG, "params[" + std::to_string(k) + "] is reserved: pass 0");
    int dims[6] = {transmittance_width, transmittance_height, multiscatter_width,
                   multiscatter_height, skyview_width,        skyview_height};
    bool all_zero = true;
    for (int k = 0; k < 6; ++k) all_zero = all_zero && dims[k] == 0;
    for (int k = 0; k < 6; ++k) {
        if (all_zero) dims[k] = kDefaultDims[k];
        if (dims[k] < 2 || dims[k] > OCEAN_ATMOSPHERE_MAX_DIM)
            return fail(OCEAN_E_INVALID_ARG, std::string(kDimNames[k]) + " = " + std::to_string(dims[k]) +
                                                 " outside [2, OCEAN_ATMOSPHERE_MAX_DIM] (all six 0: the defaults)");
    }
    OCEAN_ENTER(ctx);
    ocean_ctx::Atmosphere& a = ctx->atm;
    a.ready = a.sky_valid = a.column_valid = false;
    bool same = a.block != nullptr;
    for (int k = 0; k < 3; ++k) same = same && a.w[k] == dims[2 * k] && a.h[k] == dims[2 * k + 1];
    if (!same) {
        if (a.block) {  // launches that read the old tables may still be queued
            OCEAN_HIP(hipStreamSynchronize(ctx->stream));
            OCEAN_HIP(hipFree(a.block));
            a.block = nullptr;
        }
        size_t texels = 0;
        for (int k = 0; k < 3; ++k) texels += (size_t)dims[2 * k] * dims[2 * k + 1];
        if (hipMalloc((void**)&a.block, texels * sizeof(float4)) != hipSuccess) {
            a.block = nullptr;
            (void)hipGetLastError();
            return fail(OCEAN_E_OUT_OF_MEMORY, "hipMalloc of the atmosphere's tables failed");
        }
        float4* at = a.block;
        for (int k = 0; k < 3; ++k) {
            a.lut[k] = at;
            a.w[k] = dims[2 * k];
            a.h[k] = dims[2 * k + 1];
            at += (size_t)a.w[k] * a.h[k];
        }
    }
    std::copy(params, params + OCEAN_ATMOSPHERE_FLOATS, a.params.p);
    if (int r = timed(ctx, 2, [&] { return ocean::launch_transmittance(a.params, a.w[0], a.h[0], a.lut[0], ctx->stream); },
                      "transmittance"))
        return r;
    if (int r = timed(ctx, 2,
                      [&] { return ocean::launch_multiscatter(a.params, a.view(0), a.w[1], a.h[1], a.lut[1], ctx->stream); },
                      "multiscatter"))
        return r;
    a.ready = true;
    return OCEAN_OK;
}

int ocean_sky_update(ocean_ctx* ctx, const float* sun) {
    float n[3];
    if (int r = normalise_sun(sun, n)) return r;
    OCEAN_ENTER(ctx);
    if (int r = check_ready(ctx, "ocean_sky_update")) return r;
    ocean_ctx::Atmosphere& a = ctx->atm;
    a.sky_valid = false;
    if (int r = timed(ctx, 2,
                      [&] {
                          return ocean::launch_skyview(a.params, a.view(0), a.view(1), n, a.w[2], a.h[2], a.lut[2],
                                                       ctx->stream);
                      },
                      "skyview"))
        return r;
    a.sky_valid = true;
    return OCEAN_OK;
}

int ocean_atmosphere_read(ocean_ctx* ctx, int which, float* out, size_t bytes) {
    if (!out) return fail(OCEAN_E_INVALID_ARG, "null output");
    if (int r = check_which(which)) return r;
    OCEAN_ENTER(ctx);
    if (int r = check_ready(ctx, "ocean_atmosphere_read")) return r;
    const ocean_ctx::Atmosphere& a = ctx->atm;
    if (which == OCEAN_LUT_SKYVIEW && !a.sky_valid)
        return fail(OCEAN_E_STATE, "the sky-view table is stale: ocean_sky_update must follow ocean_atmosphere");
    const size_t want = (size_t)a.w[which] * a.h[which] * sizeof(float4);
    if (bytes != want)
        return fail(OCEAN_E_INVALID_ARG, "byte count " + std::to_string(bytes) + " != width * height * 16 = " + std::to_string(want));
    OCEAN_HIP(hipMemcpyAsync(out, a.lut[which], want, hipMemcpyDeviceToHost, ctx->stream));
    OCEAN_HIP(hipStreamSynchronize(ctx->stream));
    return OCEAN_OK;
}

int ocean_atmosphere_lut(ocean_ctx* ctx, int which, void** dev, size_t* width, size_t* height) {
    if (!dev || !width || !height) return fail(OCEAN_E_INVALID_ARG, "null dev, width or height");
    if (int r = check_which(which)) return r;
    if (!ctx) return fail(OCEAN_E_INVALID_ARG, "null context");
    if (int r = check_ready(ctx, "ocean_atmosphere_lut")) return r;
    *dev = ctx->atm.lut[which];
    *width = (size_t)ctx->atm.w[which];
    *height = (size_t)ctx->atm.h[which];
    return OCEAN_OK;
}

int ocean_sun_color(ocean_ctx* ctx, const float* sun, float* rgb) {
    if (!rgb) return fail(OCEAN_E_INVALID_ARG, "null rgb");
    float n[3];
    if (int r = normalise_sun(sun, n)) return r;
    OCEAN_ENTER(ctx);
    if (int r = check_ready(ctx, "ocean_sun_color")) return r;
    ocean_ctx::Atmosphere& a = ctx->atm;
    const int h = a.h[0];
    if (!a.column_valid) {  // column 0 of the transmittance table, once per ocean_atmosphere
        a.column.resize((size_t)h * 4);
        OCEAN_HIP(hipMemcpy2DAsync(a.column.data(), sizeof(float4), a.lut[0], (size_t)a.w[0] * sizeof(float4), sizeof(float4),
                                   (size_t)h, hipMemcpyDeviceToHost, ctx->stream));
        OCEAN_HIP(hipStreamSynchronize(ctx->stream));
        a.column_valid = true;
    }
    // TurnTransmittanceIntoColorGradient (AtmosphereController.cs:129-154): eight keys, each 2.5 x the column at t
    static const float kT[8] = {0.01f, 0.14f, 0.28f, 0.36f, 0.57f, 0.75f, 0.86f, 0.99f};
    float key[8][3];
    for (int k = 0; k < 8; ++k) {
        const float y = std::fmin(std::fmax(kT[k] * (float)h - 0.5f, 0.0f), (float)(h - 1));
        const int y0 = (int)y, y1 = std::min(y0 + 1, h - 1);
        const float f = y - (float)y0;
        for (int c = 0; c < 3; ++c) {
            const float lo = a.column[(size_t)y0 * 4 + c], hi = a.column[(size_t)y1 * 4 + c];
            key[k][c] = (lo + f * (hi - lo)) * 2.5f;
        }
    }
    // Update (:187-188): the gradient at the sun's elevation
    const float e = (n[1] + 1.0f) * 0.5f;
    if (e <= kT[0]) {
        std::copy(key[0], key[0] + 3, rgb);
    } else if (e >= kT[7]) {
        std::copy(key[7], key[7] + 3, rgb);
    } else {
        int k = 0;
        while (e >= kT[k + 1]) ++k;  // kT[k] <= e < kT[k + 1], k <= 6
        const float f = (e - kT[k]) / (kT[k + 1] - kT[k]);
        for (int c = 0; c < 3; ++c) rgb[c] = key[k][c] + f * (key[k + 1][c] - key[k][c]);
    }
    return OCEAN_OK;
}

}  // extern "C"
