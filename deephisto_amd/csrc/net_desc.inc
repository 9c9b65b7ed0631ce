// net_desc.inc -- the ONE host-side description of a ResNet patch classifier (torchvision resnet18 / resnet50 v1.5 + fc[n_cls, feat]):
// its convolutions, its residual blocks, its parameter table and its feature width.  Included in resnet_kernels.hip where the host
// side begins.  Every native engine reads it: dh_resnet18 and dh_resnet50 (infer_core.inc), the float32 trainer (train.inc) and the
// bf16 trainer (train2.inc).  An engine adds its own buffers to a conv by deriving from ConvDesc; the ORDER of an engine's parameter
// arena stays the engine's business.
namespace {

struct ConvDesc {
  std::string name;  // state_dict prefix of the conv ("layer1.0.conv1"); BN is its sibling
  std::string bn;
  int cin = 0, cout = 0, ks = 0, stride = 1;
};

// a residual block: the indices of its 2 (BasicBlock) or 3 (Bottleneck) convs in forward order, its downsample conv or -1, its stride
struct BlockDesc { int conv[3] = {-1, -1, -1}; int nconv = 0; int ds = -1; int stride = 1; };

struct NetDesc {
  std::vector<ConvDesc> convs;     // index 0 = stem; then block by block: conv1, conv2 (, conv3) (, downsample.0)
  std::vector<BlockDesc> blocks;   // forward order
  int feat = 0;                    // width of the pooled feature = fc inputs (512 / 2048)
};

NetDesc make_net_desc(bool bottleneck) {
  NetDesc d;
  auto add = [&](const std::string& n, const std::string& bn, int cin, int cout, int ks, int stride) {
    d.convs.push_back({n, bn, cin, cout, ks, stride});
    return (int)d.convs.size() - 1;
  };
  add("conv1", "bn1", 3, 64, 7, 2);
  const int width[4] = {64, 128, 256, 512}, nblk[4] = {bottleneck ? 3 : 2, bottleneck ? 4 : 2, bottleneck ? 6 : 2, bottleneck ? 3 : 2};
  int cin = 64;
  for (int s = 0; s < 4; ++s)
    for (int k = 0; k < nblk[s]; ++k) {
      const std::string pre = "layer" + std::to_string(s + 1) + "." + std::to_string(k);
      const int stride = (k == 0 && s > 0) ? 2 : 1, w = width[s], cout = bottleneck ? 4 * w : w;
      BlockDesc b;
      b.stride = stride;
      if (bottleneck) {   // torchvision v1.5: the stage stride on the 3x3 conv
        b.conv[b.nconv++] = add(pre + ".conv1", pre + ".bn1", cin, w, 1, 1);
        b.conv[b.nconv++] = add(pre + ".conv2", pre + ".bn2", w, w, 3, stride);
        b.conv[b.nconv++] = add(pre + ".conv3", pre + ".bn3", w, cout, 1, 1);
      } else {
        b.conv[b.nconv++] = add(pre + ".conv1", pre + ".bn1", cin, w, 3, stride);
        b.conv[b.nconv++] = add(pre + ".conv2", pre + ".bn2", w, w, 3, 1);
      }
      if (stride != 1 || cin != cout) b.ds = add(pre + ".downsample.0", pre + ".downsample.1", cin, cout, 1, stride);
      d.blocks.push_back(b);
      cin = cout;
    }
  d.feat = cin;
  return d;
}

// the description of "resnet18" / "resnet50", built once; null for any other name
const NetDesc* net_desc(const std::string& arch) {
  static const NetDesc r18 = make_net_desc(false), r50 = make_net_desc(true);
  return arch == "resnet18" ? &r18 : arch == "resnet50" ? &r50 : nullptr;
}

// the parameter table: elements of the state_dict entry `name` of a classifier with n_classes outputs, -1 when it has no such entry
int64_t param_elems(const NetDesc& d, int n_classes, const std::string& name) {
  if (name == "fc.weight") return (int64_t)n_classes * d.feat;
  if (name == "fc.bias") return n_classes;
  for (const auto& c : d.convs) {
    if (name == c.name + ".weight") return (int64_t)c.cout * c.cin * c.ks * c.ks;
    for (const char* s : {".weight", ".bias", ".running_mean", ".running_var"})
      if (name == c.bn + s) return c.cout;
    if (name == c.bn + ".num_batches_tracked") return 1;
  }
  return -1;
}

// a conv as the inference engines and the 3x3 launchers hold it: the description plus its device operands
struct ConvLayer : ConvDesc {
  void* w_dev = nullptr;        // packed weights
  void* w2_dev = nullptr;       // bf16 inference, stride-2 3x3 convs with cout % 128 == 0 and their downsample convs: the wide (HALF) packing
  float* scale_dev = nullptr;   // [cout]
  float* shift_dev = nullptr;
};

}  // namespace
