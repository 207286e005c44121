// host_sanitize_main.cpp -- the CPU half of the host mirror (srt_host.cpp, srt_jpeg.cpp: the loaders, the hierarchy builder, the
// flattener) run over files that tools/host_sanitize.py writes, in a build with AddressSanitizer and UBSan and without libsrt_hip.
//
//     host_sanitize LIST      LIST: one path a line; *.obj goes through loadObjFile + createBoundingHierarchy + flattenScene, anything
//                             else through load_texture.  A file the loaders refuse (false, or an exception) is a good outcome; what
//                             this program is for is the sanitizers' report, which ends the process with a non-zero status.
#include "../simple_raytracer_amd/csrc/host/srt_host.h"

#include <cstdio>
#include <exception>
#include <fstream>
#include <random>
#include <string>

using namespace srt_host;

static bool ends_with(const std::string& s, const char* tail) {
    const std::string t(tail);
    return s.size() >= t.size() && s.compare(s.size() - t.size(), t.size(), t) == 0;
}

// loaded and flattened: the flat scene must account for every triangle the object has
static bool build_and_flatten(ObjectManager& om, const std::string& name) {
    om.createBoundingHierarchy(name);
    const FlatScene f = flattenScene(&om);
    const srt_scene_desc d = f.desc();
    return d.n_tris == om.getTriangles(name).size() && f.node_left.size() == d.n_nodes;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s LIST\n", argv[0]); return 2; }
    std::ifstream list(argv[1]);
    size_t images_ok = 0, images_refused = 0, objs_ok = 0, objs_refused = 0, wrong = 0;
    for (std::string path; std::getline(list, path);) {
        if (path.empty()) continue;
        try {
            if (ends_with(path, ".obj")) {
                ObjectManager om;
                om.loadObjFile(path);
                if (!build_and_flatten(om, path)) { std::fprintf(stderr, "%s: flat scene and object disagree\n", path.c_str()); wrong++; }
                objs_ok++;
            } else {
                Texture t;
                if (!load_texture(path, t)) { images_refused++; continue; }
                if (t.dim.x <= 0 || t.dim.y <= 0 || t.rgb.size() != (size_t)t.dim.x * t.dim.y * 3) {
                    std::fprintf(stderr, "%s: %d x %d with %zu bytes\n", path.c_str(), t.dim.x, t.dim.y, t.rgb.size()); wrong++;
                }
                images_ok++;
            }
        } catch (const std::exception&) { (ends_with(path, ".obj") ? objs_refused : images_refused)++; }
    }
    // one soup made here: 20,000 triangles (above the builder's parallel-sort and task thresholds), many equal keys
    {
        std::mt19937 rng(7);
        std::uniform_real_distribution<float> u(-50.f, 50.f);
        std::vector<Triangle> tris(20000);
        for (size_t i = 0; i < tris.size(); i++) {
            const float cx = (float)(int)u(rng), cy = u(rng), cz = u(rng) - 200.f;
            tris[i].pointOne = vec4(cx, cy, cz, 1.f); tris[i].pointTwo = vec4(cx + 1.f, cy, cz, 1.f); tris[i].pointThree = vec4(cx, cy + 1.f, cz, 1.f);
        }
        ObjectManager om;
        om.setTriangles("soup", tris);
        om.objColors["soup"] = vec3(1.f, 0.f, 0.f); om.objProperties["soup"] = vec3(0.2f, 0.5f, 15.0f);
        om.transformTriangles("soup", Transformation::rotateObjY(radians(30.f)));
        if (!build_and_flatten(om, "soup")) { std::fprintf(stderr, "soup: flat scene and object disagree\n"); wrong++; }
    }
    std::printf("images: %zu decoded, %zu refused; OBJ: %zu loaded, %zu refused; soup: 20000 triangles; wrong: %zu\n",
                images_ok, images_refused, objs_ok, objs_refused, wrong);
    return wrong ? 1 : 0;
}
