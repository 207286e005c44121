// srt_host_render.cpp -- the half of the host mirror that talks to the GPU (see srt_host.h): Renderer, MultiRenderer and the drop-in
// sendRaysAndIntersectPointsColors, all through the C ABI of include/srt.h.  Everything that needs no GPU is srt_host.cpp.
#include "srt_host.h"
#include "srt_host_internal.h"

#include <stdexcept>

namespace srt_host {

// The owners, and what both renderers do with them
void SceneDestroy::operator()(srt_scene* s) const { srt_scene_destroy(s); }
void PinnedFrame::Free::operator()(uint8_t* p) const { srt_host_free(p); }
uint8_t* PinnedFrame::reserve(size_t bytes) {
    if (bytes <= bytes_) return p_.get();
    p_.reset(); bytes_ = 0;
    p_.reset((uint8_t*)srt_host_alloc(bytes));
    if (!p_) throw std::runtime_error("srt_host_alloc failed");
    bytes_ = bytes;
    return p_.get();
}

// the one place a status code of the C ABI becomes an exception: "<call>: <srt_strerror>" (Python callers see it in HostError)
static void check(int rc, const char* call) { if (rc != SRT_OK) throw std::runtime_error(std::string(call) + ": " + srt_strerror(rc)); }

// make this description resident on this device: in place when the handle's layout allows it, else a new scene
static void make_resident(SceneHandle& scene, int device, const srt_scene_desc& d) {
    const int rc = scene ? srt_scene_update(scene.get(), &d, nullptr) : SRT_ERR_LAYOUT;
    if (rc != SRT_ERR_LAYOUT) { check(rc, "srt_scene_update"); return; }
    scene.reset();
    srt_scene* fresh = nullptr;
    check(srt_scene_create(device, &d, &fresh), "srt_scene_create");
    scene.reset(fresh);
}

// a frame's srt_params: the defaults, the light staircase from lightPos.xyz and a black background; the caller adds its own fields
struct FrameParams {
    std::vector<float> lights;
    FrameParams(const vec4& lightPos, int lightAmount) : lights((size_t)lightAmount * 3) {
        const float base[3] = { lightPos.x, lightPos.y, lightPos.z };       // vec4 -> const vec3& drops w (:517 -> :405)
        srt_light_staircase(base, (uint32_t)lightAmount, lights.data());
    }
    srt_params operator()(uint32_t W, uint32_t H) const {
        srt_params p;
        srt_params_default(&p, W, H);
        p.n_lights = (uint32_t)(lights.size() / 3); p.light_pos = lights.data();      // copied by the call
        p.background[0] = p.background[1] = p.background[2] = 0;                      // ask for black so that ImageData can skip it (:518)
        return p;
    }
};

// Drop-in entry point.
// hit pixels of an 8-bit frame in the reference's emission order: x outer, y inner (:511-513).  Count per column, then fill the
// slots in parallel.  Black = "not emitted" (:518).
// `out` may come pre-sized (Renderer::collect sizes it by the previous frame's count while the GPU is still rendering: resize
// value-initialises, 20 bytes per emitted pixel of zero fill that then costs nothing on the critical path).
static void resize_both(ImageData& out, size_t n) {
    parallel_for(2, 1, [&](size_t b, size_t e) { for (size_t k = b; k < e; k++) { if (k == 0) out.imagePoints.resize(n); else out.imageColors.resize(n); } });
}
static ImageData image_data_from_rgb8(const uint8_t* rgb8, uint32_t W, uint32_t H, ImageData&& pre = ImageData()) {
    ImageData out = std::move(pre);
    std::vector<size_t> col(W + 1, 0);
    parallel_for(W, 64, [&](size_t x0, size_t x1) {
        for (size_t x = x0; x < x1; x++) {
            size_t n = 0;
            for (uint32_t y = 0; y < H; y++) { const uint8_t* c = &rgb8[((size_t)y * W + x) * 3]; n += (c[0] | c[1] | c[2]) != 0; }
            col[x + 1] = n;
        }
    });
    for (uint32_t x = 0; x < W; x++) col[x + 1] += col[x];
    if (out.imagePoints.size() < col[W] || out.imageColors.size() < col[W]) resize_both(out, col[W]);      // first frame, or more pixels than guessed
    parallel_for(W, 64, [&](size_t x0, size_t x1) {
        for (size_t x = x0; x < x1; x++) {
            size_t k = col[x];
            for (uint32_t y = 0; y < H; y++) {
                const uint8_t* c = &rgb8[((size_t)y * W + x) * 3];
                if (c[0] | c[1] | c[2]) {
                    out.imagePoints[k] = vec2((float)x, (float)y);
                    out.imageColors[k] = vec3((float)c[0], (float)c[1], (float)c[2]);
                    k++;
                }
            }
        }
    });
    if (out.imagePoints.size() != col[W]) { out.imagePoints.resize(col[W]); out.imageColors.resize(col[W]); }      // shrinking: no fill
    return out;
}

Renderer::Renderer(int device) : device_(device) {}
Renderer::~Renderer() = default;

// A sample of the per-triangle attributes the device keeps in source order (texture, texel coordinates, normals): every 61st triangle
// of every hierarchy, and the identity of the texture images.  Catches another mesh or another material under the same name and counts;
// an edit of single triangles between two frames of otherwise the same scene is NOT seen -- setFastPath(false) for such callers.
static uint64_t attribute_sample(ObjectManager* om) {
    uint64_t h = 0xcbf29ce484222325ull;
    auto mix = [&](const void* p, size_t n) { const unsigned char* c = (const unsigned char*)p; for (size_t i = 0; i < n; i++) { h ^= c[i]; h *= 0x100000001b3ull; } };
    for (const auto& pair : om->objTriangles) {
        auto hit = om->boundingVolumeHierarchy.find(pair.first);
        if (hit == om->boundingVolumeHierarchy.end()) continue;
        const std::vector<Triangle>& tr = hit->second.triangles;
        for (size_t i = 0; i < tr.size(); i += 61) {
            const Triangle& t = tr[i];
            mix(&t.normalOne, 3 * sizeof(vec3)); mix(&t.colorOneCoordinate, 3 * sizeof(vec2)); mix(t.textureName.data(), t.textureName.size());
        }
    }
    for (const auto& tx : om->textureData) {
        mix(tx.first.data(), tx.first.size()); mix(&tx.second.dim, sizeof(tx.second.dim));
        const std::vector<unsigned char>& px = tx.second.rgb;
        const size_t n = px.size();
        mix(&n, sizeof(n));
        for (size_t i = 0; i < n; i += 4099) mix(&px[i], 1);
    }
    return h;
}

// The short way (include/srt.h, f1 device half): the hierarchies' compact arrays straight to srt_scene_update_frame.  false = the
// resident scene is not this ObjectManager's (first frame, other objects or counts, other attributes): the caller takes the long way.
bool Renderer::upload_frame(ObjectManager* om) {
    if (!scene_ || !fast_path_ || sig_names_.size() != om->objTriangles.size()) return false;
    const size_t nO = sig_names_.size();
    std::vector<uint32_t> n_tris(nO), n_nodes(nO);
    std::vector<const float*> pts(nO), bmin(nO), bmax(nO);
    std::vector<const uint32_t*> ord(nO);
    std::vector<float> color(3 * nO), mat(3 * nO);
    size_t k = 0;
    for (const auto& pair : om->objTriangles) {                 // the iteration order rayIntersection:409 uses (and flattenScene)
        if (pair.first != sig_names_[k]) return false;
        auto hit = om->boundingVolumeHierarchy.find(pair.first);
        if (hit == om->boundingVolumeHierarchy.end()) return false;      // (the long way reports it)
        const ObjectManager::Hierarchy& h = hit->second;
        if (h.order.size() != sig_tris_[k] || h.nodes.size() != sig_nodes_[k] || h.points.size() != 12 * h.order.size()) return false;
        n_tris[k] = sig_tris_[k]; n_nodes[k] = sig_nodes_[k];
        pts[k] = h.points.data(); ord[k] = h.order.data(); bmin[k] = h.node_min.data(); bmax[k] = h.node_max.data();
        const vec3 c = om->objColors[pair.first], m = om->objProperties[pair.first];
        for (int a = 0; a < 3; a++) { color[3 * k + a] = c[a]; mat[3 * k + a] = m[a]; }
        k++;
    }
    if (attribute_sample(om) != sig_attr_) return false;
    srt_frame_geometry g;
    std::memset(&g, 0, sizeof(g));
    g.n_objects = (uint32_t)nO; g.obj_n_tris = n_tris.data(); g.obj_n_nodes = n_nodes.data();
    g.obj_points = pts.data(); g.obj_order = ord.data(); g.obj_node_min = bmin.data(); g.obj_node_max = bmax.data();
    g.obj_color = color.data(); g.obj_material = mat.data();
    const int rc = srt_scene_update_frame(scene_.get(), &g, nullptr);
    if (rc == SRT_ERR_LAYOUT) return false;
    check(rc, "srt_scene_update_frame");
    fast_frames_++;
    return true;
}

// the ObjectManager's current state into the device scene: the device half of the rebuild when the resident scene is this one with
// other positions (upload_frame), else flattened -- in place when the counts allow it, else a new scene
void Renderer::upload(ObjectManager* objManager) {
    pose_source_ = false;
    if (upload_frame(objManager)) return;
    FlatScene flat = flattenScene(objManager);
    make_resident(scene_, device_, flat.desc());
    // what is resident now, and its per-triangle attributes in SOURCE order for the frames that follow (the hierarchies' by-value
    // copies are in visit order: position i holds source triangle order[i])
    sig_names_ = flat.names; sig_tris_.clear(); sig_nodes_.clear();
    const size_t nt = flat.tri_obj.size();
    std::vector<float> tc(6 * nt), nrm(9 * nt);
    std::vector<int32_t> tex(nt, -1);
    bool any_tex = false;
    size_t base = 0;
    for (const std::string& name : flat.names) {
        const ObjectManager::Hierarchy& h = objManager->boundingVolumeHierarchy.at(name);
        sig_tris_.push_back((uint32_t)h.order.size()); sig_nodes_.push_back((uint32_t)h.nodes.size());
        for (size_t i = 0; i < h.order.size(); i++) {
            const size_t src = base + h.order[i], vis = base + i;
            for (int c = 0; c < 6; c++) tc[6 * src + c] = flat.tri_texcoord[6 * vis + c];
            for (int c = 0; c < 9; c++) nrm[9 * src + c] = flat.tri_normals[9 * vis + c];
            tex[src] = flat.tri_tex[vis];
            any_tex = any_tex || tex[src] >= 0;
        }
        base += h.order.size();
    }
    sig_attr_ = attribute_sample(objManager);
    const int rc = srt_scene_set_source(scene_.get(), tc.data(), nrm.data(), any_tex ? tex.data() : nullptr);
    if (rc != SRT_OK) { sig_names_.clear(); }              // no short way for this scene (it stays correct: the long way every frame)
}

void Renderer::enqueue(const vec2& imageSize, const vec4& lightPos, int lightAmount, const mat4* viewMatrix) {
    const uint32_t W = (uint32_t)imageSize.x, H = (uint32_t)imageSize.y;
    uint8_t* rgb8 = rgb8_.reserve((size_t)W * H * 3);
    const FrameParams frame(lightPos, lightAmount);
    srt_params p = frame(W, H);
    float m16[16];
    if (viewMatrix) { mat4_to_floats(*viewMatrix, m16); p.ray_matrix = m16; }
    check(srt_render_async(scene_.get(), &p, nullptr, nullptr, nullptr, rgb8), "srt_render_async");
    W_ = W; H_ = H; pending_ = true;
}

void Renderer::submit(const vec2& imageSize, const vec4& lightPos, ObjectManager* objManager, int lightAmount) {
    if (pending_) throw std::runtime_error("Renderer::submit: collect() the previous frame first");
    upload(objManager);
    enqueue(imageSize, lightPos, lightAmount, nullptr);
}

ImageData Renderer::collect() {
    if (!pending_) throw std::runtime_error("Renderer::collect: nothing submitted");
    pending_ = false;
    ImageData pre;
    if (last_count_) resize_both(pre, last_count_ + last_count_ / 16 + 64);      // while the GPU renders: the zero fill of the result vectors
    check(srt_sync(scene_.get(), nullptr), "srt_sync");
    ImageData out = image_data_from_rgb8(rgb8_.data(), W_, H_, std::move(pre));
    last_count_ = out.imagePoints.size();
    return out;
}

ImageData Renderer::render(const vec2& imageSize, const vec4& lightPos, ObjectManager* objManager, int lightAmount) {
    submit(imageSize, lightPos, objManager, lightAmount);
    return collect();
}

ImageData Renderer::renderFromCamera(const vec2& imageSize, const vec4& lightPosWorld, const mat4& viewMatrix, ObjectManager* objManager,
                                     int lightAmount, bool sceneChanged) {
    if (pending_) throw std::runtime_error("Renderer::renderFromCamera: collect() the previous frame first");
    if (!scene_ || sceneChanged) upload(objManager);
    enqueue(imageSize, lightPosWorld, lightAmount, &viewMatrix);
    return collect();
}

// POSE: the resident scene moved by one matrix per object (srt_scene_pose); nothing proportional to triangles happens on the host
// unless the scene has to be uploaded.
ImageData Renderer::renderPosed(const vec2& imageSize, const vec4& lightPos, const std::vector<mat4>& objMatrices, ObjectManager* objManager,
                                int lightAmount, bool sceneChanged) {
    if (pending_) throw std::runtime_error("Renderer::renderPosed: collect() the previous frame first");
    if (!scene_ || sceneChanged || !pose_source_) {
        upload(objManager);
        const FlatScene flat = flattenScene(objManager);       // the resident scene's visit order: the points the poses apply to
        check(srt_scene_set_pose_source(scene_.get(), flat.tri_points.data()), "srt_scene_set_pose_source");
        pose_source_ = true;
    }
    std::vector<float> m16(16 * objMatrices.size());
    for (size_t k = 0; k < objMatrices.size(); k++) mat4_to_floats(objMatrices[k], &m16[16 * k]);
    check(srt_scene_pose(scene_.get(), (uint32_t)objMatrices.size(), m16.data(), nullptr, nullptr, nullptr), "srt_scene_pose");
    enqueue(imageSize, lightPos, lightAmount, nullptr);
    return collect();
}

MultiRenderer::MultiRenderer(const std::vector<int>& devices, uint32_t blockRows) : blockRows_(blockRows ? blockRows : 8) {
    if (devices.empty()) throw std::runtime_error("MultiRenderer: no devices");
    parts_.resize(devices.size());
    for (size_t k = 0; k < devices.size(); k++) parts_[k].device = devices[k];
}
MultiRenderer::~MultiRenderer() = default;

ImageData MultiRenderer::render(const vec2& imageSize, const vec4& lightPos, ObjectManager* objManager, int lightAmount) {
    const uint32_t W = (uint32_t)imageSize.x, H = (uint32_t)imageSize.y, N = (uint32_t)parts_.size();
    FlatScene flat = flattenScene(objManager);                          // once; every device gets the same records
    const srt_scene_desc d = flat.desc();
    const FrameParams frame(lightPos, lightAmount);
    // enqueue everywhere first (upload + render + read-back on each scene's own stream), then wait
    for (uint32_t k = 0; k < N; k++) {
        Part& pt = parts_[k];
        make_resident(pt.scene, pt.device, d);
        srt_params p = frame(W, H);
        p.block_rows = blockRows_; p.block_first = k; p.block_stride = N;
        pt.rows = srt_rows_owned(&p);
        check(srt_render_async(pt.scene.get(), &p, nullptr, nullptr, nullptr, pt.rgb8.reserve((size_t)pt.rows * W * 3)), "srt_render_async");
    }
    frame_.assign((size_t)W * H * 3, 0);
    for (uint32_t k = 0; k < N; k++) {
        Part& pt = parts_[k];
        check(srt_sync(pt.scene.get(), nullptr), "srt_sync");
        for (uint32_t r = 0; r < pt.rows; r++) {                        // local row -> image row (include/srt.h srt_params)
            const uint32_t y = ((r / blockRows_) * N + k) * blockRows_ + r % blockRows_;
            std::memcpy(&frame_[(size_t)y * W * 3], pt.rgb8.data() + (size_t)r * W * 3, (size_t)W * 3);
        }
    }
    return image_data_from_rgb8(frame_.data(), W, H);
}

ImageData sendRaysAndIntersectPointsColors(const vec2& imageSize, const vec4& lightPos, ObjectManager* objManager,
                                           int lightAmount, int device) {
    // one Renderer per thread and device, kept for the life of the thread (leaked on purpose: no HIP calls from thread-exit
    // destructors): the second frame of an orbit re-uses the first frame's device scene and pinned buffers
    static thread_local std::unordered_map<int, Renderer*> renderers;
    Renderer*& r = renderers[device];
    if (!r) r = new Renderer(device);
    return r->render(imageSize, lightPos, objManager, lightAmount);
}

} // namespace srt_host
