// render_host_draw.cpp -- timing entry for the HOST drawing of the flow picture: the loops of
// HSOpticalFlowOpenCL::drawFlow / draw_cv_flow (opticalflowhs_amd/csrc/host/HSOpticalFlowOpenCL.cpp) over pnm.hpp's
// filled_circle and line, on flow planes the caller has downloaded.  tools/render_time.py times it beside
// hsflow_render_flow.   make -C tools bin/librender_host_draw.so
#include <cstdint>
#include <cstring>

#include "../opticalflowhs_amd/csrc/host/pnm.hpp"

// preset 0: the CPU route (threshold 1, half-length lines); 1: the OpenCL route (threshold 0.5, full length).
// u, v: width floats per row, dense.  rgb: 3 * width * height bytes.
extern "C" void render_host_draw(const float *u, const float *v, int W, int H, int preset, uint8_t *rgb)
{
    pnm::Image img;
    img.width = W; img.height = H; img.channels = 3;
    img.data.assign((size_t)W * H * 3, 0);
    for (int y = 0; y < H; y += 4)
        for (int x = 0; x < W; x += 4) {
            const float a = u[(size_t)y * W + x], b = v[(size_t)y * W + x];
            if (preset == 0) {
                if (a > 1 || b > 1 || a < -1 || b < -1) {
                    pnm::filled_circle(img, x, y, 2, 0, 0, 255);
                    pnm::line(img, x, y, (int)(x + a / 2), (int)(y + b / 2), 255, 0, 0);
                }
            } else if (a > 0.5f || b > 0.5f || a < -0.5f || b < -0.5f) {
                pnm::filled_circle(img, x, y, 2, 0, 0, 255);
                pnm::line(img, x, y, (int)(x + a), (int)(y + b), 255, 0, 0);
            }
        }
    std::memcpy(rgb, img.data.data(), img.data.size());
}
