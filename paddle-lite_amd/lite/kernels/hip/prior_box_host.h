// prior_box_host.h — prior_box on the host, fp32 in the reference's order of operations (lite/backends/arm/math/prior_box.cc:330-
// and the min_sizes branch of density_prior_box it calls, :234-327; ExpandAspectRatios of lite/kernels/arm/prior_box_compute.cc).
// The result depends on shapes and attributes only, so the kHIP kernel computes it once and uploads it.  No dependency beyond the
// standard library: tests compile this header into a stand-alone program and compare with the numpy oracle bit for bit.
//   min_size, max_size are truncated to int before use, as the reference does; sqrt is the float overload.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

namespace paddle {
namespace lite {
namespace kernels {
namespace hip {

// 1.0 first, then every ratio not within 1e-6 of one already there, followed by its reciprocal when flip
inline std::vector<float> ExpandAspectRatios(const std::vector<float>& in, bool flip) {
  std::vector<float> out{1.0f};
  for (float ar : in) {
    bool exists = false;
    for (float o : out)
      if (std::fabs(ar - o) < 1e-6f) {
        exists = true;
        break;
      }
    if (exists) continue;
    out.push_back(ar);
    if (flip) out.push_back(1.0f / ar);
  }
  return out;
}

inline int PriorBoxNum(const std::vector<float>& min_sizes, const std::vector<float>& max_sizes, const std::vector<float>& aspect_ratios,
                       bool flip) {
  return static_cast<int>(ExpandAspectRatios(aspect_ratios, flip).size() * min_sizes.size() + max_sizes.size());
}

// boxes, variances: [height][width][PriorBoxNum][4]; max_sizes empty or one per min_size; variance: 4 values
inline void PriorBoxHost(int height, int width, int img_height, int img_width, const std::vector<float>& min_sizes,
                         const std::vector<float>& max_sizes, const std::vector<float>& aspect_ratios, bool flip, bool clip,
                         const std::vector<float>& variance, float step_w, float step_h, float offset, bool min_max_aspect_ratios_order,
                         std::vector<float>* boxes, std::vector<float>* variances) {
  const std::vector<float> ars = ExpandAspectRatios(aspect_ratios, flip);
  const int prior_num = static_cast<int>(ars.size() * min_sizes.size() + max_sizes.size());
  if (step_w == 0 || step_h == 0) {
    step_w = static_cast<float>(img_width) / width;
    step_h = static_cast<float>(img_height) / height;
  }
  boxes->clear();
  boxes->reserve(static_cast<size_t>(height) * width * prior_num * 4);
  auto put = [&](std::vector<float>* dst, float cx, float cy, float bw, float bh) {
    dst->push_back((cx - bw / 2.f) / img_width);
    dst->push_back((cy - bh / 2.f) / img_height);
    dst->push_back((cx + bw / 2.f) / img_width);
    dst->push_back((cy + bh / 2.f) / img_height);
  };
  std::vector<float> min_buf, max_buf, com_buf;
  for (int h = 0; h < height; ++h)
    for (int w = 0; w < width; ++w) {
      const float center_x = (w + offset) * step_w;
      const float center_y = (h + offset) * step_h;
      for (size_t s = 0; s < min_sizes.size(); ++s) {
        min_buf.clear(); max_buf.clear(); com_buf.clear();
        const int min_size = static_cast<int>(min_sizes[s]);
        float bw = static_cast<float>(min_size), bh = bw;
        put(&min_buf, center_x, center_y, bw, bh);
        if (!max_sizes.empty()) {
          const int max_size = static_cast<int>(max_sizes[s]);
          bw = bh = sqrtf(static_cast<float>(min_size * max_size));
          put(&max_buf, center_x, center_y, bw, bh);
        }
        for (float ar : ars) {
          if (std::fabs(ar - 1.) < 1e-6) continue;
          bw = min_size * std::sqrt(ar);
          bh = min_size / std::sqrt(ar);
          put(&com_buf, center_x, center_y, bw, bh);
        }
        const std::vector<float>& second = min_max_aspect_ratios_order ? max_buf : com_buf;
        const std::vector<float>& third = min_max_aspect_ratios_order ? com_buf : max_buf;
        boxes->insert(boxes->end(), min_buf.begin(), min_buf.end());
        boxes->insert(boxes->end(), second.begin(), second.end());
        boxes->insert(boxes->end(), third.begin(), third.end());
      }
    }
  if (clip)
    for (float& v : *boxes) v = std::min(std::max(v, 0.f), 1.f);
  variances->resize(boxes->size());
  for (size_t i = 0; i < variances->size(); ++i) (*variances)[i] = variance[i & 3];
}

}  // namespace hip
}  // namespace kernels
}  // namespace lite
}  // namespace paddle
