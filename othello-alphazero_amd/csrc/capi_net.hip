// C ABI, the native net: its lifetime, the state_dict keys, and the host-side
// weight folding and packing for the kernels of resnet.hip.

#include <cmath>
#include <cstring>
#include <memory>

#include "capi_internal.h"

using namespace oamd;

extern "C" {

int oamd_net_create(int32_t device, const oamd_net_desc* d, oamd_net** out) {
    *out = nullptr;
    if (d->in_channels < 1 || d->in_channels > 31)
        return fail(OAMD_INVALID_ARGUMENT, "in_channels must be in [1, 31], got " + std::to_string(d->in_channels));
    if (d->conv_channels != 128 && d->conv_channels != 256)
        return fail(OAMD_INVALID_ARGUMENT,
                    "conv_channels must be 128 or 256 for the native net, got " + std::to_string(d->conv_channels));
    if (d->num_residual_blocks < 0)
        return fail(OAMD_INVALID_ARGUMENT, "num_residual_blocks must be >= 0");
    if (d->value_head_hidden_channels < 1 || d->value_head_hidden_channels > 1024)
        return fail(OAMD_INVALID_ARGUMENT, "value_head_hidden_channels must be in [1, 1024] for the native net, got " +
                                               std::to_string(d->value_head_hidden_channels));
    if (d->num_squares != 64 || d->num_actions != 65)
        return fail(OAMD_INVALID_ARGUMENT, "num_squares must be 64 and num_actions 65");
    if (d->dtype != OAMD_BF16 && d->dtype != OAMD_FP16)
        return fail(OAMD_INVALID_ARGUMENT, "dtype must be OAMD_BF16 or OAMD_FP16");
    if (int rc = create_device_checks(device)) return rc;
    DeviceGuard dg(device);  // also around the net's release on a failure below
    std::unique_ptr<oamd_net> net(new oamd_net());
    net->device = device;
    net->desc = *d;
    const int C = d->conv_channels, R = d->num_residual_blocks, hid = d->value_head_hidden_channels;
    int rc;
    if ((rc = net->w.alloc(resnet_packed_weight_alloc_elems(C, R))) ||
        (rc = net->bias.alloc((size_t)(1 + 2 * R) * C)) || (rc = net->head.alloc(resnet_head_floats(C, hid))) ||
        (rc = net->hconv.alloc(resnet_hconv_elems(C))))
        return rc;
    // state_dict keys (neural_net.py:9-172), num_batches_tracked omitted
    auto conv = [&](const std::string& p, int64_t cout, int64_t cin, int64_t k) {
        net->keys.push_back(p + ".weight");
        net->numel.push_back(cout * cin * k * k);
        net->keys.push_back(p + ".bias");
        net->numel.push_back(cout);
    };
    auto bn = [&](const std::string& p, int64_t c) {
        for (const char* s : {".weight", ".bias", ".running_mean", ".running_var"}) {
            net->keys.push_back(p + s);
            net->numel.push_back(c);
        }
    };
    auto lin = [&](const std::string& p, int64_t fin, int64_t fout) {
        net->keys.push_back(p + ".weight");
        net->numel.push_back(fin * fout);
        net->keys.push_back(p + ".bias");
        net->numel.push_back(fout);
    };
    conv("conv_block.conv", C, d->in_channels, 3);
    bn("conv_block.norm", C);
    for (int i = 0; i < R; ++i) {
        const std::string p = "residual_blocks." + std::to_string(i);
        conv(p + ".conv1", C, C, 3);
        bn(p + ".norm1", C);
        conv(p + ".conv2", C, C, 3);
        bn(p + ".norm2", C);
    }
    conv("policy_head.conv", 2, C, 1);
    bn("policy_head.norm", 2);
    lin("policy_head.linear", 128, 65);
    conv("value_head.conv", 1, C, 1);
    bn("value_head.norm", 1);
    lin("value_head.linear1", 64, hid);
    lin("value_head.linear2", hid, 1);
    *out = net.release();
    return OAMD_OK;
}

int oamd_net_destroy(oamd_net* net) {
    if (!net) return OAMD_OK;
    DeviceGuard dg(net->device);
    delete net;
    return OAMD_OK;
}

int oamd_net_state_size(const oamd_net* net, int32_t* n) {
    *n = (int32_t)net->keys.size();
    return OAMD_OK;
}

int oamd_net_state_key(const oamd_net* net, int32_t i, const char** key, int64_t* numel) {
    if (i < 0 || i >= (int32_t)net->keys.size()) return fail(OAMD_OUT_OF_RANGE, "state index out of range");
    *key = net->keys[i].c_str();
    *numel = net->numel[i];
    return OAMD_OK;
}

static uint16_t f32_to_bf16_rne(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

static uint16_t f32_to_f16(float f) {
    _Float16 h = (_Float16)f;
    uint16_t u;
    std::memcpy(&u, &h, 2);
    return u;
}

int oamd_net_load_state(oamd_net* net, const float* const* t, int32_t n_tensors) {
    if (n_tensors != (int32_t)net->keys.size())
        return fail(OAMD_INVALID_ARGUMENT, "expected " + std::to_string(net->keys.size()) + " tensors, got " +
                                               std::to_string(n_tensors));
    const auto& d = net->desc;
    const int C = d.conv_channels, R = d.num_residual_blocks, hid = d.value_head_hidden_channels;
    const double eps = 1e-5;  // torch.nn.BatchNorm2d default
    int ti = 0;
    std::vector<uint16_t> packed(resnet_packed_weight_elems(C, R));
    std::vector<float> bias((size_t)(1 + 2 * R) * C);
    size_t ks_global = 0;
    // fold BN into a 3x3 conv and pack in MFMA A-fragment order, K-step by K-step
    // (resnet_kstep): [ks][ntile][lane][8]; lane holds output channel
    // resnet_out_channel(ntile, lane&15) and input channels cb*32 + 8*chunk(lane>>4) + j
    auto pack_conv = [&](int layer, int cin, bool first) {
        const float* W = t[ti++];
        const float* b = t[ti++];
        const float* g = t[ti++];
        const float* be = t[ti++];
        const float* mu = t[ti++];
        const float* var = t[ti++];
        std::vector<double> scale(C);
        for (int n = 0; n < C; ++n) {
            scale[n] = (double)g[n] / std::sqrt((double)var[n] + eps);
            bias[(size_t)layer * C + n] = (float)(((double)b[n] - (double)mu[n]) * scale[n] + (double)be[n]);
        }
        const int nk = resnet_ksteps(C, first);
        for (int i = 0; i < nk; ++i) {
            int tap, cb;
            bool pad;
            resnet_kstep(C, first, i, &tap, &cb, &pad);
            const size_t ks = ks_global + (size_t)i;
            for (int nt = 0; nt < C / 16; ++nt)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int ci = cb * 32 + 8 * resnet_kgroup_chunk(lane >> 4) + j;
                        const int n = resnet_out_channel(nt, lane & 15);
                        double v = 0.0;
                        if (!pad && ci < cin) v = (double)W[((size_t)n * cin + ci) * 9 + tap] * scale[n];
                        const size_t idx = (((ks * (C / 16) + nt) * 64) + lane) * 8 + j;
                        packed[idx] = d.dtype == OAMD_BF16 ? f32_to_bf16_rne((float)v) : f32_to_f16((float)v);
                    }
        }
        ks_global += (size_t)nk;
    };
    pack_conv(0, d.in_channels, true);
    for (int i = 0; i < R; ++i) {
        pack_conv(1 + 2 * i, C, false);
        pack_conv(2 + 2 * i, C, false);
    }
    // heads (fp32; 1x1 conv + BN folded)
    std::vector<float> head(resnet_head_floats(C, hid));
    // the offsets of resnet.hip's HeadLayout, restated (the other copy)
    const int HL_pcw = 0, HL_pcb = HL_pcw + 2 * C, HL_vcw = HL_pcb + 2, HL_vcb = HL_vcw + C,
              HL_plw = HL_vcb + 1, HL_plb = HL_plw + 128 * 65, HL_v1w = HL_plb + 65, HL_v1b = HL_v1w + 64 * hid,
              HL_v2w = HL_v1b + hid, HL_v2b = HL_v2w + hid;
    {
        const float* W = t[ti++];
        const float* b = t[ti++];
        const float* g = t[ti++];
        const float* be = t[ti++];
        const float* mu = t[ti++];
        const float* var = t[ti++];
        for (int c = 0; c < 2; ++c) {
            const double s = (double)g[c] / std::sqrt((double)var[c] + eps);
            for (int ch = 0; ch < C; ++ch) head[HL_pcw + c * C + ch] = (float)((double)W[c * C + ch] * s);
            head[HL_pcb + c] = (float)(((double)b[c] - (double)mu[c]) * s + (double)be[c]);
        }
        const float* LW = t[ti++];
        const float* LB = t[ti++];
        for (int a = 0; a < 65; ++a) {
            for (int i = 0; i < 128; ++i) head[HL_plw + i * 65 + a] = LW[a * 128 + i];
            head[HL_plb + a] = LB[a];
        }
    }
    {
        const float* W = t[ti++];
        const float* b = t[ti++];
        const float* g = t[ti++];
        const float* be = t[ti++];
        const float* mu = t[ti++];
        const float* var = t[ti++];
        const double s = (double)g[0] / std::sqrt((double)var[0] + eps);
        for (int ch = 0; ch < C; ++ch) head[HL_vcw + ch] = (float)((double)W[ch] * s);
        head[HL_vcb] = (float)(((double)b[0] - (double)mu[0]) * s + (double)be[0]);
        const float* W1 = t[ti++];
        const float* B1 = t[ti++];
        for (int j = 0; j < hid; ++j) {
            for (int sq = 0; sq < 64; ++sq) head[HL_v1w + sq * hid + j] = W1[j * 64 + sq];
            head[HL_v1b + j] = B1[j];
        }
        const float* W2 = t[ti++];
        const float* B2 = t[ti++];
        for (int j = 0; j < hid; ++j) head[HL_v2w + j] = W2[j];
        head[HL_v2b] = B2[0];
    }
    // 1x1 head convs (folded) in MFMA A-fragment order: lane holds row lane&15
    // (0, 1 = policy channels, 2 = value, else 0) and input channels
    // cb*32 + 8*chunk(lane>>4) + j, matching the tower's B fragments
    std::vector<uint16_t> hconv(resnet_hconv_elems(C));
    for (int cb = 0; cb < C / 32; ++cb)
        for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 8; ++j) {
                const int r = lane & 15, ci = cb * 32 + 8 * resnet_kgroup_chunk(lane >> 4) + j;
                const float v = r < 2 ? head[HL_pcw + r * C + ci] : (r == 2 ? head[HL_vcw + ci] : 0.0f);
                hconv[((size_t)cb * 64 + lane) * 8 + j] = d.dtype == OAMD_BF16 ? f32_to_bf16_rne(v) : f32_to_f16(v);
            }
    DeviceGuard dg(net->device);
    // searches run the ResNet on non-blocking streams, which a plain hipMemcpy
    // does not order against: let every launch still reading these buffers
    // finish before they are overwritten (a weight refresh between searches)
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(net->hconv.get(), hconv.data(), hconv.size() * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(net->w.get(), packed.data(), packed.size() * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(net->w.get() + packed.size(), 0,
                     (resnet_packed_weight_alloc_elems(C, R) - packed.size()) * sizeof(uint16_t)));
    HIPCHK(hipMemcpy(net->bias.get(), bias.data(), bias.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(net->head.get(), head.data(), head.size() * 4, hipMemcpyHostToDevice));
    net->loaded = true;
    return OAMD_OK;
}

int oamd_net_forward(oamd_net* net, const float* features, int32_t rows, float* policy, float* value,
                     void* stream) {
    if (!net->loaded) return fail(OAMD_INVALID_ARGUMENT, "net weights not loaded");
    if (rows < 0) return fail(OAMD_INVALID_ARGUMENT, "rows must be >= 0");
    DeviceGuard dg(net->device);
    launch_resnet_f32(net->view(), features, rows, policy, value, (hipStream_t)stream);
    LAUNCHCHK();
    return OAMD_OK;
}

int oamd_debug_forward_packed(oamd_net* net, const uint64_t* feat_dev, int64_t feat_rows, int32_t history,
                              const int32_t* list_host, int32_t list_len, int32_t count, int32_t list_off,
                              int32_t rows, int32_t max_wgs, float* policy_dev, float* value_dev, int64_t out_rows,
                              void* stream) {
    if (!net || !net->loaded) return fail(OAMD_INVALID_ARGUMENT, "forward_packed: net weights not loaded");
    if (history < 1 || history > kMaxHistory)
        return fail(OAMD_INVALID_ARGUMENT, "forward_packed: history must be in [1, 15], got " + std::to_string(history));
    if (net->desc.in_channels != 1 + 2 * history)
        return fail(OAMD_INVALID_ARGUMENT, "forward_packed: net in_channels != 1 + 2 * history");
    if (feat_rows < 0 || out_rows < 0 || rows < 0 || max_wgs < 0 || count < 0)
        return fail(OAMD_INVALID_ARGUMENT, "forward_packed: negative size");
    // every row a launch can read or write lies below this
    const int64_t bound = std::min(feat_rows, out_rows);
    if (list_host) {
        if (list_len < 0 || list_off < 0 || (int64_t)list_off + rows > (int64_t)list_len)
            return fail(OAMD_INVALID_ARGUMENT, "forward_packed: list_off + rows exceeds list_len");
        for (int32_t i = 0; i < list_len; ++i)
            if (list_host[i] < 0 || list_host[i] >= bound)
                return fail(OAMD_INVALID_ARGUMENT, "forward_packed: list entry " + std::to_string(i) + " = " +
                                                       std::to_string(list_host[i]) + " is not a row of both buffers");
    } else {
        if (list_len != 0 || list_off != 0)
            return fail(OAMD_INVALID_ARGUMENT, "forward_packed: list_len and list_off must be 0 without a list");
        if (rows > bound) return fail(OAMD_INVALID_ARGUMENT, "forward_packed: rows exceeds feat_rows or out_rows");
    }
    if (rows == 0) return OAMD_OK;
    if (!feat_dev || !policy_dev || !value_dev) return fail(OAMD_INVALID_ARGUMENT, "forward_packed: null buffer");
    DeviceGuard dg(net->device);
    const int32_t* list_dev = nullptr;
    const int32_t* count_dev = nullptr;
    if (list_host) {
        // the previous call's launch may still read the list (any stream)
        HIPCHK(hipDeviceSynchronize());
        if ((int64_t)list_len + 1 > net->debug_list_cap) {
            net->debug_list_cap = 0;
            if (int rc = net->debug_list.alloc((size_t)list_len + 1)) return rc;
            net->debug_list_cap = (int64_t)list_len + 1;
        }
        // [0] the counter, [1 ..] the list
        HIPCHK(hipMemcpy(net->debug_list.get(), &count, sizeof(int32_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(net->debug_list.get() + 1, list_host, (size_t)list_len * sizeof(int32_t),
                         hipMemcpyHostToDevice));
        HIPCHK(hipDeviceSynchronize());
        count_dev = net->debug_list.get();
        list_dev = net->debug_list.get() + 1 + list_off;
    }
    launch_resnet_packed(net->view(), feat_dev, feature_words(history), history, rows, policy_dev, value_dev,
                         (hipStream_t)stream, list_dev, count_dev, list_off, nullptr, max_wgs);
    LAUNCHCHK();
    return OAMD_OK;
}

}  // extern "C"
