// infer_core.inc -- what the two inference engines (dh_resnet18 in resnet_kernels.hip, dh_resnet50 in resnet50_infer.inc) share on the
// host: the handle's common state, the parameter entry, the checks and uploads of finalize, the workspace, the tiles / tap / operands
// entries and the tap itself.  It plays the part on the inference side that train_core.inc plays on the training side.  Included in
// resnet_kernels.hip behind the packers and conv launchers it calls, in front of dh_resnet18 and its forward.
//
// An engine keeps what genuinely differs: how it packs a conv's operands at finalize (ResNet-18: scale and shift per conv, three stem
// packings, the wide stride-2 second packing; ResNet-50: BN folded into the weights), its forward, and its InferEngine: its name in
// messages, its argument limits (a function: the two engines' limits and texts differ) and two facts about its operands.  Nothing here
// branches on which engine called.  The forward comes in as a callable that takes the Tap* (null: a plain forward); whatever an
// engine does between the argument checks and its launches -- ResNet-50 reads the origins back and checks them, ResNet-18 does not,
// which keeps a host wait off its path -- is part of that callable.
namespace {

struct InferNet {
  int n_classes = 0;
  const NetDesc* desc = nullptr;                     // net_desc.inc: blocks and feature width; `convs` below follows desc->convs
  std::map<std::string, std::vector<float>> params;  // host copies by state_dict name
  std::vector<ConvLayer> convs;                      // index 0 = stem
  float* fc_w_dev = nullptr;
  float* fc_b_dev = nullptr;
  bool finalized = false;
  void* ws = nullptr;                                // activation workspace, sized for the largest launch shape so far
  size_t ws_bytes = 0;
};

struct InferEngine {
  const char* name;   // "resnet18" / "resnet50": the prefix of every message
  // handle, finalized flag and the engine's limits on (n, P); `out` is the entry's mandatory output, `what` names the entry
  int (*check)(const InferNet* net, int64_t n, int32_t P, const void* out, const char* what);
  int feat_align;     // features_tiles: alignment of feat_dev in bytes the engine's head kernel needs (1: none)
  bool plain_1x1;     // 1x1 weights are held as plain bf16 [cout][cin] (gemm1x1_infer.inc), not in fragment order
};

template <typename V>
int upload(const std::vector<V>& v, void** dev) {
  if (*dev) { DH_HIP(hipFree(*dev)); *dev = nullptr; }
  DH_HIP(hipMalloc(dev, v.size() * sizeof(V)));
  DH_HIP(hipMemcpy(*dev, v.data(), v.size() * sizeof(V), hipMemcpyHostToDevice));
  return DH_OK;
}

void infer_init(InferNet* net, const char* arch, int n_classes) {
  net->n_classes = n_classes;
  net->desc = net_desc(arch);
  for (const ConvDesc& d : net->desc->convs) net->convs.push_back(ConvLayer{d});
}

// frees the device memory every handle owns (an engine frees what it adds, then deletes the handle)
void infer_free(InferNet* net) {
  for (auto& c : net->convs) {
    if (c.w_dev) (void)hipFree(c.w_dev);
    if (c.w2_dev) (void)hipFree(c.w2_dev);
    if (c.scale_dev) (void)hipFree(c.scale_dev);
    if (c.shift_dev) (void)hipFree(c.shift_dev);
  }
  if (net->fc_w_dev) (void)hipFree(net->fc_w_dev);
  if (net->fc_b_dev) (void)hipFree(net->fc_b_dev);
  if (net->ws) (void)hipFree(net->ws);
}

int infer_set_param(const InferEngine& e, InferNet* net, const char* name, const float* data, int64_t n_elem) {
  DH_REQUIRE(net && name && data, "%s set_param: null argument", e.name);
  const int64_t want = param_elems(*net->desc, net->n_classes, name);
  DH_REQUIRE(want >= 0, "%s set_param: unknown parameter '%s'", e.name, name);
  DH_REQUIRE(want == n_elem, "%s set_param: '%s' has %lld elements, expected %lld", e.name, name, (long long)n_elem, (long long)want);
  net->params[name].assign(data, data + n_elem);
  net->finalized = false;
  return DH_OK;
}

inline const std::vector<float>* infer_param(const InferNet* net, const std::string& key) {
  auto it = net->params.find(key);
  return it == net->params.end() ? nullptr : &it->second;
}

// First step of finalize: the handle stops being finalized, then every tensor of every conv and the fc must be present -- BEFORE any
// upload, so that a failed finalize never leaves a handle with some layers replaced.
int infer_finalize_begin(const InferEngine& e, InferNet* net) {
  DH_REQUIRE(net != nullptr, "%s finalize: null handle", e.name);
  net->finalized = false;
  for (const auto& c : net->convs)
    DH_REQUIRE(infer_param(net, c.name + ".weight") && infer_param(net, c.bn + ".weight") && infer_param(net, c.bn + ".bias") &&
               infer_param(net, c.bn + ".running_mean") && infer_param(net, c.bn + ".running_var"),
               "%s finalize: parameters of '%s' / '%s' are not all set", e.name, c.name.c_str(), c.bn.c_str());
  DH_REQUIRE(infer_param(net, "fc.weight") && infer_param(net, "fc.bias"), "%s finalize: fc.weight / fc.bias are not set", e.name);
  return DH_OK;
}

// eval-mode BN (eps = 1e-5, torch default) of conv `c` in float64: y = x * scale + shift
void infer_bn_affine(const InferNet* net, const ConvLayer& c, std::vector<double>& scale, std::vector<double>& shift) {
  const auto &g = *infer_param(net, c.bn + ".weight"), &b = *infer_param(net, c.bn + ".bias"), &m = *infer_param(net, c.bn + ".running_mean"),
             &v = *infer_param(net, c.bn + ".running_var");
  scale.resize(c.cout); shift.resize(c.cout);
  for (int k = 0; k < c.cout; ++k) {
    const double s = (double)g[k] / sqrt((double)v[k] + 1e-5);
    scale[k] = s;
    shift[k] = (double)b[k] - (double)m[k] * s;
  }
}

// Last step of finalize: the fc operands (float32 in both engines); the handle is finalized from here on
int infer_finalize_end(InferNet* net) {
  int rc;
  if ((rc = upload(*infer_param(net, "fc.weight"), reinterpret_cast<void**>(&net->fc_w_dev))) ||
      (rc = upload(*infer_param(net, "fc.bias"), reinterpret_cast<void**>(&net->fc_b_dev)))) return rc;
  net->finalized = true;
  return DH_OK;
}

// grows the workspace to `need` bytes (it never shrinks)
int infer_workspace(InferNet* net, size_t need) {
  if (need > net->ws_bytes) {
    if (net->ws) DH_HIP(hipFree(net->ws));
    net->ws = nullptr; net->ws_bytes = 0;
    DH_HIP(hipMalloc(&net->ws, need));
    net->ws_bytes = need;
  }
  return DH_OK;
}

// Test hook of the inference forwards (dh_debug_resnet18_forward_tap, dh_debug_resnet50_forward_tap): right after the launch that stores
// conv `name`'s output, that buffer's images sel[0..k) as float32 NCHW [k][C][H][W], stream-ordered before any later launch can overwrite
// it.  A forward without a tap (nullptr) issues exactly its own launches.
struct Tap {
  std::string name;
  const int32_t* sel = nullptr;   // device, checked against the launch's n by the hook
  int k = 0;
  float* out = nullptr;
  int64_t out_elems = 0;
  bool hit = false;
};

// in: [image][C/cp][H][W][cp] -- cp = 32: channel-blocked, 16: 16-channel planes, C: NHWC
template <typename T>
__global__ void tap_gather_kernel(const T* __restrict__ in, const int32_t* __restrict__ sel, int C, int cp, int64_t hw, int64_t total,
                                  float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t px = i % hw;
    const int c = (int)((i / hw) % C);
    const int64_t b = sel[i / hw / C];
    out[i] = (float)in[((b * (C / cp) + c / cp) * hw + px) * cp + c % cp];
  }
}

template <typename T>
int tap_after(Tap* tap, const std::string& name, const void* buf, int C, int H, int W, int cp, hipStream_t st) {
  if (!tap || name != tap->name) return DH_OK;
  const int64_t total = (int64_t)tap->k * C * H * W;
  DH_REQUIRE(total == tap->out_elems, "forward tap %s: the output holds %lld elements, [%d][%d][%d][%d] needs %lld", name.c_str(),
             (long long)tap->out_elems, tap->k, C, H, W, (long long)total);
  hipLaunchKernelGGL((tap_gather_kernel<T>), dim3((unsigned)std::min<int64_t>((total + 255) / 256, 4096)), dim3(256), 0, st,
                     static_cast<const T*>(buf), tap->sel, C, cp, (int64_t)H * W, total, tap->out);
  DH_LAUNCH_CHECK();
  tap->hit = true;
  return DH_OK;
}

// Host checks of a tap request before any launch: k in [1, n], every sel in [0, n) (read back: one synchronisation of `st`)
int tap_check(const int32_t* sel_dev, int32_t k, int64_t n, float* out_dev, const float* logits_dev, hipStream_t st) {
  DH_REQUIRE(sel_dev && out_dev && logits_dev, "forward tap: null argument");
  DH_REQUIRE(k > 0 && k <= n, "forward tap: k = %d selected images out of range [1, %lld]", k, (long long)n);
  std::vector<int32_t> sel(k);
  DH_HIP(hipMemcpyAsync(sel.data(), sel_dev, (size_t)k * 4, hipMemcpyDeviceToHost, st));
  DH_HIP(hipStreamSynchronize(st));
  for (int i = 0; i < k; ++i)
    DH_REQUIRE(sel[i] >= 0 && sel[i] < n, "forward tap: sel[%d] = %d outside the launch of %lld tiles", i, sel[i], (long long)n);
  return DH_OK;
}

// the stored activations a tap may name: every conv of the topology, and "maxpool" (the pooled stem output)
bool tap_name_known(const InferNet* net, const char* name) {
  if (!strcmp(name, "maxpool")) return true;
  for (const auto& c : net->convs)
    if (c.name == name) return true;
  return false;
}

// The fused gather + forward behind forward_tiles and features_tiles: the argument checks, then the engine's forward.  `what` names
// the entry in messages; `feat` (features_tiles: the pooled vector of every tile, the tap one step before the logits) may be null;
// `out` is the entry's mandatory output.
template <typename Fwd>
int infer_tiles(const InferEngine& e, InferNet* net, const uint8_t* slide, int64_t h, int64_t w, const int32_t* yx, int64_t n, int32_t P,
                const float* feat, const float* out, const char* what, Fwd&& forward) {
  if (int rc = e.check(net, n, P, out, what)) return rc;
  if (n == 0) return DH_OK;
  DH_REQUIRE(slide && yx, "%s: null slide or origins", what);
  DH_REQUIRE(reinterpret_cast<uintptr_t>(feat) % e.feat_align == 0, "%s: feat_dev is not %d-byte aligned", what, e.feat_align);
  DH_REQUIRE(h >= P && w >= P, "%s: patch %d does not fit %lldx%lld", what, P, (long long)h, (long long)w);
  return forward(static_cast<Tap*>(nullptr));
}

// The tap entry: the forward of forward_tiles with one stored activation copied out (Tap above)
template <typename Fwd>
int infer_tap(const InferEngine& e, InferNet* net, const uint8_t* slide, int64_t h, int64_t w, const int32_t* yx_dev, int64_t n, int32_t P,
              const char* conv_name, const int32_t* sel_dev, int32_t k, float* out_dev, int64_t out_elems, float* logits_dev,
              hipStream_t st, Fwd&& forward) {
  const std::string what = std::string(e.name) + " forward tap";
  if (int rc = e.check(net, n, P, logits_dev, what.c_str())) return rc;
  DH_REQUIRE(n > 0 && slide && yx_dev && conv_name, "%s: null argument or empty launch", what.c_str());
  DH_REQUIRE(h >= P && w >= P, "%s: patch %d does not fit %lldx%lld", what.c_str(), P, (long long)h, (long long)w);
  DH_REQUIRE(tap_name_known(net, conv_name), "%s: unknown conv '%s'", what.c_str(), conv_name);
  if (int rc = tap_check(sel_dev, k, n, out_dev, logits_dev, st)) return rc;
  Tap tap;
  tap.name = conv_name; tap.sel = sel_dev; tap.k = k; tap.out = out_dev; tap.out_elems = out_elems;
  if (int rc = forward(&tap)) return rc;
  DH_REQUIRE(tap.hit, "%s: '%s' is not stored by this engine", what.c_str(), conv_name);
  return DH_OK;
}

// a conv's operands as the engine holds them: the packed weight read back from the device and unpacked, scale and shift (or 1 and the
// folded bias) read back; synchronous
int read_operands(const ConvLayer& c, int esz, bool fused_stem, float* w_host, int64_t w_elems, float* scale_host, float* shift_host,
                  int64_t c_elems) {
  DH_REQUIRE(w_host && scale_host && shift_host, "operands: null argument");
  DH_REQUIRE(w_elems == (int64_t)c.cout * c.cin * c.ks * c.ks && c_elems == c.cout, "operands %s: buffers of %lld / %lld elements, "
             "expected %lld / %d", c.name.c_str(), (long long)w_elems, (long long)c_elems, (long long)c.cout * c.cin * c.ks * c.ks, c.cout);
  size_t bytes;
  if (c.ks == 7) bytes = fused_stem ? (size_t)SP_WBYTES : (size_t)7 * 11 * 2 * 256;
  else bytes = (size_t)(c.cout / 64) * (c.cin / (CHUNK_BYTES / esz)) * c.ks * c.ks * SLAB_TAP;
  std::vector<uint8_t> packed(bytes);
  DH_HIP(hipMemcpy(packed.data(), c.w_dev, bytes, hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < w_elems; ++i) w_host[i] = NAN;   // an element no slot carries stays NaN
  if (c.ks == 7 && fused_stem) unpack_stem_pool_weights(packed, w_host);
  else if (c.ks == 7) unpack_stem_weights_f32(packed, w_host);
  else unpack_conv_weights(packed, c.cout, c.cin, c.ks, esz, w_host);
  DH_HIP(hipMemcpy(scale_host, c.scale_dev, (size_t)c.cout * 4, hipMemcpyDeviceToHost));
  DH_HIP(hipMemcpy(shift_host, c.shift_dev, (size_t)c.cout * 4, hipMemcpyDeviceToHost));
  return DH_OK;
}

// The operands entry: conv `conv_name`'s operands as the engine holds them after finalize, `esz` bytes per weight element (2: bf16, which
// runs the fused stem)
int infer_operands(const InferEngine& e, const InferNet* net, int esz, const char* conv_name, float* w_host, int64_t w_elems,
                   float* scale_host, float* shift_host, int64_t c_elems) {
  DH_REQUIRE(net && net->finalized && conv_name, "%s operands: needs a finalized network", e.name);
  for (const auto& c : net->convs) {
    if (c.name != conv_name) continue;
    if (!(e.plain_1x1 && c.ks == 1)) return read_operands(c, esz, esz == 2, w_host, w_elems, scale_host, shift_host, c_elems);
    DH_REQUIRE(w_host && scale_host && shift_host && w_elems == (int64_t)c.cout * c.cin && c_elems == c.cout,
               "%s operands %s: bad buffers", e.name, c.name.c_str());
    std::vector<uint16_t> wb((size_t)w_elems);   // gemm1x1_infer.inc's W operand: plain bf16 [cout][cin]
    DH_HIP(hipMemcpy(wb.data(), c.w_dev, wb.size() * 2, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < w_elems; ++i) {
      const uint32_t u = (uint32_t)wb[i] << 16;
      memcpy(&w_host[i], &u, 4);
    }
    DH_HIP(hipMemcpy(scale_host, c.scale_dev, (size_t)c.cout * 4, hipMemcpyDeviceToHost));
    DH_HIP(hipMemcpy(shift_host, c.shift_dev, (size_t)c.cout * 4, hipMemcpyDeviceToHost));
    return DH_OK;
  }
  dh::set_error("%s operands: unknown conv '%s'", e.name, conv_name);
  return DH_EINVAL;
}

}  // namespace
