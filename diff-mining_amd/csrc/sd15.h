// sd15.h — architecture constants of the public SDv1.5 checkpoint (unet / vae / text_encoder config.json), once, for the fp16 engine
// (engine*.hip) and the fp32 net (f32_*.hip).
#pragma once

namespace sd15 {

constexpr int NB = 4;
const int BOC[NB] = {320, 640, 1280, 1280};
constexpr int LAYERS = 2;
constexpr int CTX_DIM = 768;
constexpr int CTX_LEN = 77;
constexpr int HEADS = 8;
constexpr int GROUPS = 32;
constexpr int TEMB = 1280;
constexpr int NTRAIN = 1000;
constexpr float GN_EPS = 1e-5f, ATTN_GN_EPS = 1e-6f, LN_EPS = 1e-5f;
const bool DOWN_ATTN[NB] = {true, true, true, false};
const bool UP_ATTN[NB] = {false, true, true, true};

// SDv1.5 VAE encoder (block_out_channels 128/256/512/512, two resnets per block, no time embedding)
constexpr int VNB = 4;
const int VBOC[VNB] = {128, 256, 512, 512};
constexpr float VAE_EPS = 1e-6f;

// CLIP ViT-L/14 text tower (12 pre-LN layers, hidden 768, 12 heads of 64, MLP 3072 quick_gelu)
constexpr int CL_LAYERS = 12, CL_H = 768, CL_F = 3072, CL_HEADS = 12, CL_T = 77, CL_VOCAB = 49408;

}  // namespace sd15
