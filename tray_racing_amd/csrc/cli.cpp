// cli.cpp — `tray_racing_hip`: the reference's command line (src/main.rs:65-171) over the C ABI.
//
// Same flag names and the same 4-column result table (src/main.rs:634-640, printed once after
// `--passes` passes, averaged: :188-207).  What differs is the backend: every frame is the primary +
// AO frame of src/rt_gpu/rt_gpu_software.hlsl:47-144 traced by libtrx.so on an MI355X; the BVH is
// built on the CPU by this repo's stand-in builder (the reference builds with OBVHS).  Links against
// include/trx.h only.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <sstream>
#include <string>
#include <vector>

#include <zlib.h>

#include "../../include/trx.h"

namespace {

struct Options { // src/main.rs:65-171 (flags this backend cannot honour are rejected loudly)
    std::string input;
    bool benchmark = false;
    float render_time = 1.0f;
    std::string build = "ploc_cwbvh";
    unsigned max_prims_per_leaf = 3;
    bool cpu = false, hardware = false, verbose = false, animate = false, png = false, tlas = false, flatten_blas = false;
    unsigned width = 1920, height = 1080;
    float collapse_traversal_cost = 1.0f;
    unsigned passes = 3;
    std::string preset;
    float reinsertion_batch_ratio = 0.15f; // -r (src/main.rs:113-118)
    unsigned search_distance = 14, search_depth_threshold = 2, sort_precision = 64; // src/main.rs:85-98,110-112
    float post_collapse_multiplier = 0.0f;
    bool dry_run = false; // load + build only (no device needed)
    bool gpu_build = false; // --gpu-build: Morton sort + PLOC rounds of the build on the device (trx_set_build_device)
    bool split = false;   // --split: pre-splitting of large triangles
    bool overlap = false; // --overlap: frame i's AO pass under frame i + 1's primary pass (trx_frame_loop, two streams)
    // --ao-samples N / --ao-radius R: with --png, the image's AO term is count / N of the AO visibility pass
    // (trx_trace_ao_visibility) instead of t / (1 + t); either flag switches it on (N defaults to 1, R to +inf)
    unsigned ao_samples = 0;
    float ao_radius = 0.0f;
    // --ao-filter R [--ao-depth-tol x] [--ao-normal-cos c]: with --png --ao-samples N the image is made on the device
    // (trx_render_image): the counts through the edge-aware filter of radius R (0: unfiltered), shaded to RGBA8 there
    int ao_filter = -1; // -1: not given, save_png's host loop stays as it is
    float ao_depth_tol = 0.02f, ao_normal_cos = 0.9f;
    // --profile-rt nodes|tris [--profile-rt-scale x]: with --png the image is the PROFILE_RT heat map (trx_render_heat_image)
    // --ao-stride S [--ao-phase P] [--ao-upsample R]: with --png --ao-samples N the AO term is traced at one pixel in S x S
    // and rebuilt at full resolution by the edge-aware upsample of radius R (trx_render_image_sparse), on the device
    int ao_stride = -1; // -1: not given, everything stays as it is
    int ao_phase = -1, ao_upsample = -1; // (not given: phase 0, radius 1)
    int profile_rt = -1; // -1: not given, else TRX_HEAT_NODES / TRX_HEAT_TRIS
    float profile_rt_scale = -1.0f; // (not given: the reference's scale of the mode)
    // --light point:x,y,z[:i] | dir:x,y,z[:i] | rect:cx,cy,cz:ax,ay,az:bx,by,bz[:i] (repeatable): with --png the image is the
    // direct-light image (trx_render_image_lit): shadow rays toward every light, --light-samples N of them per rect light, cast
    // with ray mask --light-mask M (0: unmasked) from --shadow-eps e behind the hit; --ambient a is scaled by the AO term of
    // --ao-samples / --ao-filter when those are given
    std::vector<trx_light> lights;
    int light_samples = -1, light_mask = -1; // (not given: 1 sample, unmasked)
    float shadow_eps = -1.0f, ambient = -1.0f; // (not given: 0.01, 0.1)
    // --bounce-samples N [--bounce-albedo a] [--bounce-eps e]: with --png --light the image is the GI image
    // (trx_render_image_gi): the direct-light image plus one diffuse bounce of N samples per pixel
    int bounce_samples = -1; // -1: not given, everything stays as it is
    float bounce_albedo = -1.0f, bounce_eps = -1.0f; // (not given: 0.5, 0.01)
    // --bounce-filter L [--bounce-filter-tol d] [--bounce-filter-cos c]: with --bounce-samples the bounce's term goes through L
    // levels of the edge-aware value filter before it is added (trx_render_image_gi_filtered)
    int bounce_filter = -1; // -1: not given, everything stays as it is
    float bounce_filter_tol = 0.1f, bounce_filter_cos = 0.9f;
    bool bounce_filter_opts = false; // one of the two tolerances was given
    // --bounce-stride S [--bounce-phase P] [--bounce-upsample R]: with --bounce-samples the bounce's term is traced at one pixel
    // in S x S and rebuilt by the edge-aware upsample (trx_render_image_gi_sparse; the filter's two tolerances are its own)
    int bounce_stride = -1; // -1: not given, everything stays as it is
    int bounce_phase = -1, bounce_upsample = -1; // (not given: phase 0, radius 1)
    // --colour: with --png --light the image is the colour image (trx_render_image_colour) - the scene gets a material table, the
    // mtl files' for -i <file.obj>, the stand-in table for standin:<name>, and every --bounce-*, --ao-* and --light option applies
    bool colour = false;
    // --emitters N [--emitter-eps e]: with --png --colour the image is trx_render_image_colour_emitters' - the scene's emissive
    // triangles sampled as lights, N shadow rays per pixel toward them (and one per bounce ray), each stopped e of its length
    // short of the emitter; --light becomes optional
    int emitters = -1;
    float emitter_eps = -1.0f;
    // --smooth [--smooth-crease DEG]: with --png --light (the direct-light image) or with --colour the light term and the filters
    // shade with interpolated vertex normals (trx_render_image_lit_smooth / _colour_smooth) - the OBJ's `vn` records where the
    // file has any, else normals computed from the mesh, welded across edges flatter than DEG degrees (default 45)
    bool smooth = false;
    float smooth_crease = -1.0f; // (not given: 45)
    // --textures: with --png --colour the image is trx_render_image_colour_textured's - texcoords and albedo textures from the
    // OBJ's `vt` and the mtl files' map_Kd (binary PPM or 8-bit PNG, taken as sRGB, bilinear) for -i <file.obj>, the stand-in
    // tables for standin:<name>; goes with --emitters and with --smooth
    bool textures = false;
    int device = 0;
    unsigned semantics = TRX_SEM_HLSL; // the GPU path of the reference is the HLSL text
};

struct Camera {
    float eye[3] = {0, 0, 0}, look_at[3] = {0, 0, -1}, fov = 90.0f;
};

struct Stats {
    std::string name;
    double traversal_ms = 0, blas_build_time_s = 0, tlas_build_time_ms = 0;
};

[[noreturn]] void die(const std::string &msg) {
    std::fprintf(stderr, "%s\n", msg.c_str());
    std::exit(1);
}

void check(int rc, const char *what) {
    if (rc != TRX_OK) die(std::string(what) + ": " + trx_last_error());
}

void usage() {
    std::puts("tray_racing_hip -i <scene.ron|demoscene|standin:<name>>[,...] [--benchmark] [--render-time s]\n"
              "  [--build ploc_cwbvh] [--max-prims-per-leaf 1..3] [--collapse-traversal-cost c] [--preset p]\n"
              "  [--width w] [--height h] [--animate] [--tlas] [--flatten-blas] [--passes n] [--verbose] [--device d]\n"
              "  [--png] [--cpu-semantics] [--dry-run (load + build only, needs no GPU)] [-r reinsertion_batch_ratio]\n"
              "  [--search-distance d] [--search-depth-threshold n] [--sort-precision 64|128] [--split] [--gpu-build]\n"
              "  [--overlap (frames stay on the device, frame i's AO pass under frame i+1's primary pass; reports the average)]\n"
              "  [--ao-samples 1..64] [--ao-radius r] (with --png: AO term = unoccluded samples / N of the any-hit visibility pass)\n"
              "  [--ao-filter 0..4] [--ao-depth-tol x] [--ao-normal-cos c] (with --png --ao-samples: edge-aware filter of that radius\n"
              "   over the AO counts, image shaded on the device; only the RGBA8 bytes are copied back)\n"
              "  [--ao-stride 1..4] [--ao-phase 0..S*S-1] [--ao-upsample 0..2] (with --png --ao-samples: AO rays at one pixel in\n"
              "   S x S, the full-resolution term by the edge-aware upsample of that radius (default 1) under --ao-depth-tol and\n"
              "   --ao-normal-cos, image shaded on the device; not together with --ao-filter)\n"
              "  [--profile-rt nodes|tris] [--profile-rt-scale x] (with --png: the PROFILE_RT heat map of a counted primary pass -\n"
              "   box tests (8 per node visit) x 0.002 or triangle tests x 0.01 through the reference's colour ramp - instead of\n"
              "   the shaded frame; not together with --ao-samples or --ao-filter)\n"
              "  [--light point:x,y,z[:i] | dir:x,y,z[:i] | rect:cx,cy,cz:ax,ay,az:bx,by,bz[:i]] (repeatable, up to 8; with --png: the\n"
              "   direct-light image - shadow rays toward every light, intensity i (default 1) - shaded on the device)\n"
              "  [--light-samples 1..64] [--light-mask 0..255] [--shadow-eps e] [--ambient a] (with --light: samples per rect light,\n"
              "   the shadow rays' instance mask, their offset, the ambient term - scaled by the AO term of --ao-samples /\n"
              "   --ao-filter; not together with --ao-stride or --profile-rt)\n"
              "  [--bounce-samples 1..64] [--bounce-albedo a] [--bounce-eps e] (with --png --light: one diffuse bounce - N bounce rays\n"
              "   per pixel, the direct light at what they hit times the albedo (default 0.5), added to the direct-light image;\n"
              "   not together with --ao-stride or --profile-rt)\n"
              "  [--bounce-filter 0..5] [--bounce-filter-tol d] [--bounce-filter-cos c] (with --bounce-samples: the bounce's term through\n"
              "   L levels of the edge-aware a-trous filter - taps 1, 2, 4, .. pixels apart, kept where the depth is within d (default\n"
              "   0.1) of the pixel's and the normals within c (default 0.9) - before it is added; 0: unfiltered)\n"
              "  [--bounce-stride 1..4] [--bounce-phase P] [--bounce-upsample 0..2] (with --bounce-samples: the bounce rays of one pixel\n"
              "   in every S x S block - pixel P = 0..S*S-1 of the block, default 0 - and the full-resolution term rebuilt from the\n"
              "   cells of a (2R+1)^2 window, default R = 1, under --bounce-filter-tol / --bounce-filter-cos; before --bounce-filter)\n"
              "  [--colour] (with --png --light: the colour image - per-triangle albedo and emission from the mtl files of\n"
              "   -i <file.obj> or the stand-in table of standin:<name>; the bounce carries the colour of what it hit; not together\n"
              "   with --bounce-albedo)\n"
              "  [--emitters 1..64] [--emitter-eps e] (with --png --colour: the emissive triangles sampled as lights - N shadow rays per\n"
              "   pixel and one per bounce ray toward points on them, each stopped e (default 0.001) of its length short of the\n"
              "   emitter; --light becomes optional)\n"
              "  [--textures] (with --png --colour, also with --emitters or --smooth: albedo textures - the `vt` of -i <file.obj> and the\n"
              "   map_Kd files of its mtl files, binary PPM (P6, maxval 255) or 8-bit non-interlaced RGB / RGBA PNG, read as sRGB and\n"
              "   filtered bilinearly; the box mapping and the checker of standin:<name>; not without --colour, with --benchmark or\n"
              "   with --profile-rt)\n"
              "  [--smooth] [--smooth-crease DEG] (with --png --light or with --colour: shade with interpolated vertex normals - the\n"
              "   `vn` records of -i <file.obj> where it has any, else computed from the mesh, corners welded across edges flatter\n"
              "   than DEG degrees, default 45; rays still start from the geometric normal; not together with --bounce-samples\n"
              "   without --colour, --emitters, --profile-rt or --benchmark)\n"
              "stand-in names: cornell demoscene kitchen bistro hairball san_miguel (seeded procedural scenes)");
}

// point:x,y,z[:i] | dir:x,y,z[:i] | rect:cx,cy,cz:ax,ay,az:bx,by,bz[:i]
trx_light parse_light(const std::string &text) {
    const std::string form = "--light takes point:x,y,z[:i], dir:x,y,z[:i] or rect:cx,cy,cz:ax,ay,az:bx,by,bz[:i]";
    std::vector<std::string> parts;
    for (size_t at = 0;;) {
        const size_t colon = text.find(':', at);
        parts.push_back(text.substr(at, colon == std::string::npos ? colon : colon - at));
        if (colon == std::string::npos) break;
        at = colon + 1;
    }
    trx_light l;
    std::memset(&l, 0, sizeof(l));
    l.intensity = 1.0f;
    size_t vectors = 1;
    if (parts[0] == "point") l.kind = TRX_LIGHT_POINT;
    else if (parts[0] == "dir") l.kind = TRX_LIGHT_DIRECTIONAL;
    else if (parts[0] == "rect") l.kind = TRX_LIGHT_RECT, vectors = 3;
    else die(form);
    if (parts.size() != 1 + vectors && parts.size() != 2 + vectors) die(form);
    auto number = [&](const std::string &t) {
        char *end = nullptr;
        const float x = std::strtof(t.c_str(), &end);
        if (t.empty() || *end != '\0' || !std::isfinite(x)) die(form);
        return x;
    };
    float *dst[3] = {l.position, l.edge1, l.edge2};
    for (size_t v = 0; v < vectors; v++) {
        const std::string &t = parts[1 + v];
        const size_t c1 = t.find(','), c2 = c1 == std::string::npos ? c1 : t.find(',', c1 + 1);
        if (c2 == std::string::npos || t.find(',', c2 + 1) != std::string::npos) die(form);
        dst[v][0] = number(t.substr(0, c1));
        dst[v][1] = number(t.substr(c1 + 1, c2 - c1 - 1));
        dst[v][2] = number(t.substr(c2 + 1));
    }
    if (parts.size() == 2 + vectors) l.intensity = number(parts[1 + vectors]);
    if (l.kind == TRX_LIGHT_DIRECTIONAL && l.position[0] == 0.0f && l.position[1] == 0.0f && l.position[2] == 0.0f)
        die("--light dir: takes a direction of non-zero length");
    return l;
}

Options parse_args(int argc, char **argv) {
    Options o;
    auto need = [&](int &i) -> const char * {
        if (i + 1 >= argc) die(std::string("missing value for ") + argv[i]);
        return argv[++i];
    };
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        if (a == "-i") o.input = need(i);
        else if (a == "--benchmark") o.benchmark = true;
        else if (a == "--render-time") o.render_time = (float)std::atof(need(i));
        else if (a == "--build") o.build = need(i);
        else if (a == "--max-prims-per-leaf") o.max_prims_per_leaf = (unsigned)std::atoi(need(i));
        else if (a == "--collapse-traversal-cost") o.collapse_traversal_cost = (float)std::atof(need(i));
        else if (a == "--preset") o.preset = need(i);
        else if (a == "--width") o.width = (unsigned)std::atoi(need(i));
        else if (a == "--height") o.height = (unsigned)std::atoi(need(i));
        else if (a == "--passes") o.passes = (unsigned)std::atoi(need(i));
        else if (a == "--device") o.device = std::atoi(need(i));
        else if (a == "--cpu") o.cpu = true;
        else if (a == "--hardware") o.hardware = true;
        else if (a == "--verbose") o.verbose = true;
        else if (a == "--animate") o.animate = true;
        else if (a == "--png") o.png = true;
        else if (a == "--tlas") o.tlas = true;
        else if (a == "--flatten-blas") o.flatten_blas = true;
        else if (a == "--cpu-semantics") o.semantics = TRX_SEM_CPU;
        else if (a == "--dry-run") o.dry_run = true;
        else if (a == "--gpu-build") o.gpu_build = true;
        else if (a == "--overlap") o.overlap = true;
        else if (a == "--ao-samples") {
            o.ao_samples = (unsigned)std::atoi(need(i));
            if (o.ao_samples == 0 || o.ao_samples > TRX_MAX_AO_SAMPLES) die("--ao-samples takes 1.." + std::to_string(TRX_MAX_AO_SAMPLES));
        } else if (a == "--ao-radius") {
            o.ao_radius = (float)std::atof(need(i));
            if (!(o.ao_radius > 0.0f)) die("--ao-radius must be > 0");
        }
        else if (a == "--ao-filter") {
            o.ao_filter = std::atoi(need(i));
            if (o.ao_filter < 0 || o.ao_filter > TRX_MAX_AO_FILTER_RADIUS) die("--ao-filter takes 0.." + std::to_string(TRX_MAX_AO_FILTER_RADIUS));
        } else if (a == "--ao-depth-tol") {
            o.ao_depth_tol = (float)std::atof(need(i));
            if (!(o.ao_depth_tol >= 0.0f)) die("--ao-depth-tol must be >= 0");
        } else if (a == "--ao-normal-cos") {
            o.ao_normal_cos = (float)std::atof(need(i));
            if (o.ao_normal_cos != o.ao_normal_cos) die("--ao-normal-cos must be a number");
        }
        else if (a == "--ao-stride") {
            o.ao_stride = std::atoi(need(i));
            if (o.ao_stride < 1 || o.ao_stride > TRX_MAX_AO_STRIDE) die("--ao-stride takes 1.." + std::to_string(TRX_MAX_AO_STRIDE));
        } else if (a == "--ao-phase") {
            o.ao_phase = std::atoi(need(i));
            if (o.ao_phase < 0) die("--ao-phase takes 0..S*S-1 of --ao-stride S");
        } else if (a == "--ao-upsample") {
            o.ao_upsample = std::atoi(need(i));
            if (o.ao_upsample < 0 || o.ao_upsample > TRX_MAX_AO_UPSAMPLE_RADIUS) die("--ao-upsample takes 0.." + std::to_string(TRX_MAX_AO_UPSAMPLE_RADIUS));
        }
        else if (a == "--light") {
            if (o.lights.size() >= TRX_MAX_LIGHTS) die("--light: at most " + std::to_string(TRX_MAX_LIGHTS) + " lights");
            o.lights.push_back(parse_light(need(i)));
        } else if (a == "--light-samples") {
            o.light_samples = std::atoi(need(i));
            if (o.light_samples < 1 || o.light_samples > TRX_MAX_AO_SAMPLES) die("--light-samples takes 1.." + std::to_string(TRX_MAX_AO_SAMPLES));
        } else if (a == "--light-mask") {
            o.light_mask = std::atoi(need(i));
            if (o.light_mask < 0 || o.light_mask > 255) die("--light-mask takes 0..255");
        } else if (a == "--shadow-eps") {
            o.shadow_eps = (float)std::atof(need(i));
            if (!(o.shadow_eps >= 0.0f)) die("--shadow-eps must be >= 0");
        } else if (a == "--ambient") {
            o.ambient = (float)std::atof(need(i));
            if (!(o.ambient >= 0.0f) || !std::isfinite(o.ambient)) die("--ambient must be finite and >= 0");
        }
        else if (a == "--bounce-samples") {
            o.bounce_samples = std::atoi(need(i));
            if (o.bounce_samples < 1 || o.bounce_samples > TRX_MAX_AO_SAMPLES) die("--bounce-samples takes 1.." + std::to_string(TRX_MAX_AO_SAMPLES));
        } else if (a == "--bounce-albedo") {
            o.bounce_albedo = (float)std::atof(need(i));
            if (!(o.bounce_albedo >= 0.0f) || !std::isfinite(o.bounce_albedo)) die("--bounce-albedo must be finite and >= 0");
        } else if (a == "--bounce-eps") {
            o.bounce_eps = (float)std::atof(need(i));
            if (!(o.bounce_eps >= 0.0f)) die("--bounce-eps must be >= 0");
        } else if (a == "--bounce-filter") {
            o.bounce_filter = std::atoi(need(i));
            if (o.bounce_filter < 0 || o.bounce_filter > TRX_MAX_VALUE_FILTER_LEVELS) die("--bounce-filter takes 0.." + std::to_string(TRX_MAX_VALUE_FILTER_LEVELS));
        } else if (a == "--bounce-stride") {
            o.bounce_stride = std::atoi(need(i));
            if (o.bounce_stride < 1 || o.bounce_stride > TRX_MAX_AO_STRIDE) die("--bounce-stride takes 1.." + std::to_string(TRX_MAX_AO_STRIDE));
        } else if (a == "--bounce-phase") {
            o.bounce_phase = std::atoi(need(i));
            if (o.bounce_phase < 0) die("--bounce-phase takes 0..S*S-1 of --bounce-stride S");
        } else if (a == "--bounce-upsample") {
            o.bounce_upsample = std::atoi(need(i));
            if (o.bounce_upsample < 0 || o.bounce_upsample > TRX_MAX_VALUE_UPSAMPLE_RADIUS)
                die("--bounce-upsample takes 0.." + std::to_string(TRX_MAX_VALUE_UPSAMPLE_RADIUS));
        } else if (a == "--bounce-filter-tol") {
            o.bounce_filter_tol = (float)std::atof(need(i));
            o.bounce_filter_opts = true;
            if (!(o.bounce_filter_tol >= 0.0f)) die("--bounce-filter-tol must be >= 0");
        } else if (a == "--bounce-filter-cos") {
            o.bounce_filter_cos = (float)std::atof(need(i));
            o.bounce_filter_opts = true;
            if (o.bounce_filter_cos != o.bounce_filter_cos) die("--bounce-filter-cos must be a number");
        }
        else if (a == "--colour") {
            o.colour = true;
        } else if (a == "--emitters") {
            o.emitters = std::atoi(need(i));
            if (o.emitters < 1 || o.emitters > TRX_MAX_AO_SAMPLES) die("--emitters takes 1.." + std::to_string(TRX_MAX_AO_SAMPLES));
        } else if (a == "--emitter-eps") {
            o.emitter_eps = (float)std::atof(need(i));
            if (!(o.emitter_eps >= 0.0f && o.emitter_eps < 1.0f)) die("--emitter-eps takes a number in [0, 1)");
        }
        else if (a == "--smooth") {
            o.smooth = true;
        } else if (a == "--textures") {
            o.textures = true;
        } else if (a == "--smooth-crease") {
            o.smooth_crease = (float)std::atof(need(i));
            if (!(o.smooth_crease >= 0.0f && o.smooth_crease <= 180.0f)) die("--smooth-crease takes an angle of 0..180 degrees");
        }
        else if (a == "--profile-rt") {
            const std::string m = need(i);
            if (m == "nodes") o.profile_rt = (int)TRX_HEAT_NODES;
            else if (m == "tris") o.profile_rt = (int)TRX_HEAT_TRIS;
            else die("--profile-rt takes nodes or tris");
        } else if (a == "--profile-rt-scale") {
            o.profile_rt_scale = (float)std::atof(need(i));
            if (!(o.profile_rt_scale >= 0.0f) || o.profile_rt_scale > std::numeric_limits<float>::max()) die("--profile-rt-scale must be finite and >= 0");
        }
        else if (a == "-h" || a == "--help") {
            usage();
            std::exit(0);
        } else if (a == "-r") {
            o.reinsertion_batch_ratio = (float)std::atof(need(i));
        } else if (a == "--search-distance") {
            o.search_distance = (unsigned)std::atoi(need(i));
        } else if (a == "--search-depth-threshold") {
            o.search_depth_threshold = (unsigned)std::atoi(need(i));
        } else if (a == "--sort-precision") {
            o.sort_precision = (unsigned)std::atoi(need(i));
        } else if (a == "--post-collapse-reinsertion-batch-ratio-multiplier") {
            o.post_collapse_multiplier = (float)std::atof(need(i)); // "For BVH2 only" (src/main.rs:119-123)
        } else if (a == "--split") {
            o.split = true;
        } else if (a == "--auto-tune" || a == "--disable-auto-tune-model-cache") {
            // accepted for command-line compatibility; no effect here
        } else {
            die("unknown argument: " + a);
        }
    }
    if (o.input.empty()) {
        usage();
        die("error: -i <input> is required");
    }
    if (o.build.find("cwbvh") != std::string::npos && o.max_prims_per_leaf > 3)
        die("CWBVH only supports a maximum of 3 primitives per leaf."); // src/main.rs:176-178
    if (o.build != "ploc_cwbvh") die("NO BVH BUILDER SPECIFIED (this backend serves --build ploc_cwbvh)"); // src/cwbvh.rs:99
    if (o.cpu) die("--cpu is the reference's own rt_cpu path; the HIP backend has no CPU traversal");
    if (o.hardware) die("--hardware needs ray-tracing hardware; MI355X (CDNA4) has none");
    if (o.ao_filter >= 0 && o.ao_samples == 0) die("--ao-filter filters the counts of --ao-samples N");
    if (o.ao_stride < 0 && (o.ao_phase >= 0 || o.ao_upsample >= 0)) die("--ao-phase and --ao-upsample go with --ao-stride S");
    if (o.ao_stride >= 0 && o.ao_samples == 0) die("--ao-stride thins the rays of --ao-samples N");
    if (o.ao_stride >= 0 && o.ao_filter >= 0) die("--ao-stride rebuilds the term with --ao-upsample: not together with --ao-filter");
    if (o.ao_stride >= 0 && o.ao_phase >= o.ao_stride * o.ao_stride) die("--ao-phase takes 0..S*S-1 of --ao-stride S");
    if (o.profile_rt >= 0 && (o.ao_samples != 0 || o.ao_filter >= 0)) die("--profile-rt draws the heat map: not together with --ao-samples or --ao-filter");
    if (o.profile_rt < 0 && o.profile_rt_scale >= 0.0f) die("--profile-rt-scale scales the heat map of --profile-rt nodes|tris");
    if (o.emitters < 0 && o.emitter_eps >= 0.0f) die("--emitter-eps goes with --emitters N");
    if (o.emitters >= 0 && !o.colour) die("--emitters samples the emissive materials of --colour");
    if (o.emitters >= 0 && !o.png) die("--emitters lights the image of --png");
    if (o.emitters >= 0 && (o.ao_stride >= 0 || o.profile_rt >= 0)) die("--emitters draws the colour image: not together with --ao-stride or --profile-rt");
    if (o.lights.empty() && o.emitters < 0 && (o.light_samples >= 0 || o.light_mask >= 0 || o.shadow_eps >= 0.0f || o.ambient >= 0.0f))
        die("--light-samples, --light-mask, --shadow-eps and --ambient go with --light");
    if (!o.lights.empty() && !o.png) die("--light lights the image of --png");
    if (!o.lights.empty() && (o.ao_stride >= 0 || o.profile_rt >= 0)) die("--light draws the direct-light image: not together with --ao-stride or --profile-rt");
    if (o.bounce_samples < 0 && (o.bounce_albedo >= 0.0f || o.bounce_eps >= 0.0f)) die("--bounce-albedo and --bounce-eps go with --bounce-samples N");
    if (o.bounce_samples >= 0 && (o.ao_stride >= 0 || o.profile_rt >= 0)) die("--bounce-samples draws the GI image: not together with --ao-stride or --profile-rt");
    if (o.bounce_samples >= 0 && o.lights.empty() && o.emitters < 0) die("--bounce-samples bounces the light of --light");
    if (o.bounce_stride < 0 && (o.bounce_phase >= 0 || o.bounce_upsample >= 0)) die("--bounce-phase and --bounce-upsample go with --bounce-stride S");
    if (o.bounce_stride >= 0 && o.bounce_samples < 0) die("--bounce-stride thins the rays of --bounce-samples N");
    if (o.bounce_stride >= 0 && o.bounce_phase >= o.bounce_stride * o.bounce_stride) die("--bounce-phase takes 0..S*S-1 of --bounce-stride S");
    if (o.bounce_filter < 0 && o.bounce_stride < 0 && o.bounce_filter_opts) die("--bounce-filter-tol and --bounce-filter-cos go with --bounce-filter L");
    if (o.bounce_filter >= 0 && o.bounce_samples < 0) die("--bounce-filter filters the term of --bounce-samples N");
    if (o.colour && o.lights.empty() && o.emitters < 0) die("--colour colours the image of --light");
    if (o.colour && o.bounce_albedo >= 0.0f) die("--colour takes the albedo of the materials: not together with --bounce-albedo");
    if (o.textures && !o.colour) die("--textures textures the image of --colour");
    if (o.textures && o.benchmark) die("--textures textures the image of --png: not together with --benchmark");
    if (o.textures && o.profile_rt >= 0) die("--textures textures the colour image: not together with --profile-rt");
    if (!o.smooth && o.smooth_crease >= 0.0f) die("--smooth-crease goes with --smooth");
    if (o.smooth && o.benchmark) die("--smooth shades the image of --png: not together with --benchmark");
    if (o.smooth && o.profile_rt >= 0) die("--smooth shades the lit image: not together with --profile-rt");
    if (o.smooth && o.emitters >= 0) die("--smooth shades the image of --light or --colour: not together with --emitters");
    if (o.smooth && o.bounce_samples >= 0 && !o.colour) die("--smooth shades the direct-light image or the colour image: not together with the grey --bounce-samples image");
    if (o.smooth && (!o.png || o.lights.empty())) die("--smooth shades the image of --png --light or of --colour");
    if (o.passes == 0) o.passes = 1;
    return o;
}

// 8-bit RGBA PNG, one zlib stream, filter 0 on every scanline
void put_be32(std::vector<unsigned char> &v, uint32_t x) {
    for (int k = 3; k >= 0; k--) v.push_back((unsigned char)(x >> (8 * k)));
}
void png_chunk(std::ofstream &f, const char *tag, const std::vector<unsigned char> &body) {
    std::vector<unsigned char> head, crc_in(tag, tag + 4);
    put_be32(head, (uint32_t)body.size());
    crc_in.insert(crc_in.end(), body.begin(), body.end());
    std::vector<unsigned char> tail;
    put_be32(tail, (uint32_t)crc32(0L, crc_in.data(), (uInt)crc_in.size()));
    f.write((const char *)head.data(), 4);
    f.write((const char *)crc_in.data(), (std::streamsize)crc_in.size());
    f.write((const char *)tail.data(), 4);
}
bool write_png(const std::string &path, const std::vector<unsigned char> &rgba, unsigned w, unsigned h) {
    std::vector<unsigned char> raw;
    raw.reserve((size_t)h * (w * 4 + 1));
    for (unsigned y = 0; y < h; y++) {
        raw.push_back(0);
        raw.insert(raw.end(), rgba.begin() + (size_t)y * w * 4, rgba.begin() + (size_t)(y + 1) * w * 4);
    }
    uLongf zlen = compressBound((uLong)raw.size());
    std::vector<unsigned char> z(zlen);
    if (compress2(z.data(), &zlen, raw.data(), (uLong)raw.size(), 6) != Z_OK) return false;
    z.resize(zlen);
    std::ofstream f(path, std::ios::binary);
    if (!f) return false;
    const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    f.write((const char *)sig, 8);
    std::vector<unsigned char> ihdr;
    put_be32(ihdr, w);
    put_be32(ihdr, h);
    const unsigned char fmt[5] = {8, 6, 0, 0, 0}; // 8 bit, RGBA
    ihdr.insert(ihdr.end(), fmt, fmt + 5);
    png_chunk(f, "IHDR", ihdr);
    png_chunk(f, "IDAT", z);
    png_chunk(f, "IEND", {});
    return (bool)f;
}

// ---- image files for --textures: decoded here, the library stays free of decoders.  Both give RGBA8 words (R in the low
// byte), row 0 the TOP row of the image as the file has it; false = not such a file (the caller says so and goes on).

// binary PPM: "P6", width, height, maxval 255 (blank-separated, `#` comments to the end of their line), one blank, then RGB bytes
bool read_ppm(const std::vector<unsigned char> &d, std::vector<uint32_t> &px, uint32_t &w, uint32_t &h) {
    if (d.size() < 2 || d[0] != 'P' || d[1] != '6') return false;
    size_t p = 2;
    unsigned long num[3] = {0, 0, 0};
    for (int k = 0; k < 3; k++) {
        for (;;) { // blanks and comments
            while (p < d.size() && (d[p] == ' ' || d[p] == '\t' || d[p] == '\n' || d[p] == '\r')) p++;
            if (p < d.size() && d[p] == '#') {
                while (p < d.size() && d[p] != '\n') p++;
                continue;
            }
            break;
        }
        const size_t start = p;
        while (p < d.size() && d[p] >= '0' && d[p] <= '9' && p - start < 9) num[k] = num[k] * 10 + (d[p++] - '0');
        if (p == start) return false;
    }
    if (p >= d.size() || !(d[p] == ' ' || d[p] == '\t' || d[p] == '\n' || d[p] == '\r')) return false;
    p++;
    if (num[0] == 0 || num[1] == 0 || num[0] > TRX_MAX_TEXTURE_SIZE || num[1] > TRX_MAX_TEXTURE_SIZE || num[2] != 255) return false;
    const size_t n = (size_t)num[0] * num[1];
    if (d.size() - p < n * 3) return false;
    w = (uint32_t)num[0], h = (uint32_t)num[1];
    px.resize(n);
    for (size_t i = 0; i < n; i++) px[i] = d[p + 3 * i] | (uint32_t)d[p + 3 * i + 1] << 8 | (uint32_t)d[p + 3 * i + 2] << 16 | 0xFF000000u;
    return true;
}

// PNG: 8 bits per channel, colour type 2 (RGB) or 6 (RGBA), not interlaced; the IDAT chunks are one zlib stream (the zlib this
// program links for its own PNG), every scanline one filter byte and the five filters of the PNG specification
bool read_png(const std::vector<unsigned char> &d, std::vector<uint32_t> &px, uint32_t &w, uint32_t &h) {
    static const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    if (d.size() < 8 || std::memcmp(d.data(), sig, 8) != 0) return false;
    auto be32 = [&](size_t at) { return (uint32_t)d[at] << 24 | (uint32_t)d[at + 1] << 16 | (uint32_t)d[at + 2] << 8 | (uint32_t)d[at + 3]; };
    size_t p = 8;
    std::vector<unsigned char> z;
    uint32_t bpp = 0;
    bool header = false, end = false;
    while (!end && d.size() - p >= 12) {
        const uint32_t len = be32(p);
        if (len > d.size() - p - 12) return false;
        const unsigned char *tag = &d[p + 4], *body = &d[p + 8];
        if (std::memcmp(tag, "IHDR", 4) == 0) {
            if (len != 13 || header) return false;
            w = be32(p + 8), h = be32(p + 12);
            if (w == 0 || h == 0 || w > TRX_MAX_TEXTURE_SIZE || h > TRX_MAX_TEXTURE_SIZE) return false;
            if (body[8] != 8 || (body[9] != 2 && body[9] != 6) || body[10] != 0 || body[11] != 0 || body[12] != 0) return false;
            bpp = body[9] == 2 ? 3u : 4u;
            header = true;
        } else if (std::memcmp(tag, "IDAT", 4) == 0) {
            if (!header) return false;
            z.insert(z.end(), body, body + len);
        } else if (std::memcmp(tag, "IEND", 4) == 0) {
            end = true;
        }
        p += (size_t)len + 12;
    }
    if (!header || !end || z.empty()) return false;
    const size_t stride = (size_t)w * bpp;
    std::vector<unsigned char> raw((stride + 1) * h);
    uLongf got = (uLongf)raw.size();
    if (uncompress(raw.data(), &got, z.data(), (uLong)z.size()) != Z_OK || got != raw.size()) return false;
    std::vector<unsigned char> prev(stride, 0), cur(stride);
    px.resize((size_t)w * h);
    for (uint32_t y = 0; y < h; y++) {
        const unsigned char *line = &raw[(stride + 1) * y];
        const unsigned filter = line[0];
        if (filter > 4) return false;
        for (size_t i = 0; i < stride; i++) {
            const int a = i >= bpp ? cur[i - bpp] : 0, b = prev[i], c = i >= bpp ? prev[i - bpp] : 0; // left, up, up-left
            int pred = 0;
            if (filter == 1) pred = a;
            else if (filter == 2) pred = b;
            else if (filter == 3) pred = (a + b) / 2;
            else if (filter == 4) {
                const int pa = std::abs(b - c), pb = std::abs(a - c), pc = std::abs(a + b - 2 * c);
                pred = pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
            }
            cur[i] = (unsigned char)(line[1 + i] + pred);
        }
        for (uint32_t x = 0; x < w; x++) {
            const unsigned char *q = &cur[(size_t)x * bpp];
            px[(size_t)y * w + x] = q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (bpp == 4 ? (uint32_t)q[3] << 24 : 0xFF000000u);
        }
        prev.swap(cur);
    }
    return true;
}

// an image file of --textures: PPM or PNG by its first bytes; a message on stderr and false for anything else
bool read_image(const std::string &path, std::vector<uint32_t> &px, uint32_t &w, uint32_t &h) {
    std::ifstream f(path, std::ios::binary);
    std::vector<unsigned char> d;
    if (f) d.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    if (!f || d.empty()) {
        std::fprintf(stderr, "--textures: cannot read %s: its material stays untextured\n", path.c_str());
        return false;
    }
    if (read_ppm(d, px, w, h) || read_png(d, px, w, h)) return true;
    std::fprintf(stderr, "--textures: %s is neither a binary PPM (P6, maxval 255) nor an 8-bit non-interlaced RGB / RGBA PNG: its material stays untextured\n",
                 path.c_str());
    return false;
}

// The reference's image: AO term of the primary hit, 1/t where the primary ray missed, gamma 2.2 to u8
// (src/rt_cpu/rt_cpu.rs:57-85,102-112; the same shading ends the GPU shader, rt_gpu_software.hlsl:47-144).
void save_png(const Options &o, trx_scene *scene, const trx_view &view, unsigned frame_count, const std::string &name) {
    const size_t n = (size_t)o.width * o.height;
    std::vector<unsigned char> rgba(n * 4);
    const std::string path = name + "_rend.png";
    float ms = 0;
    if (o.profile_rt >= 0) {
        // where the tree is expensive: the per-ray counts of a counted primary pass as colours, made on the device
        const float scale = o.profile_rt_scale >= 0.0f ? o.profile_rt_scale : o.profile_rt == (int)TRX_HEAT_TRIS ? TRX_HEAT_SCALE_TRIS : TRX_HEAT_SCALE_NODES;
        trx_stats st;
        check(trx_render_heat_image(scene, &view, o.width, o.height, o.semantics, (uint32_t)o.profile_rt, scale, rgba.data(), &st), "heat map");
        if (!write_png(path, rgba, o.width, o.height)) die("Failed to save image " + path);
        if (o.verbose)
            std::printf("saved %s (heat map of %s, scale %g: %.2f node visits, %.2f triangle tests per ray)\n", path.c_str(),
                        o.profile_rt == (int)TRX_HEAT_TRIS ? "triangle tests" : "box tests", (double)scale,
                        (double)st.n_node / (double)std::max<uint64_t>(st.n_rays, 1), (double)st.n_tri / (double)std::max<uint64_t>(st.n_rays, 1));
        return;
    }
    if (!o.lights.empty() || o.emitters >= 0) {
        // the direct-light image, made on the device: shadow rays, the light term, the value shade; 4 bytes per pixel back
        const bool ao = o.ao_samples != 0 || o.ao_radius > 0.0f;
        const unsigned ao_samples = o.ao_samples ? o.ao_samples : ao ? 1u : 0u;
        const float radius = o.ao_radius > 0.0f ? o.ao_radius : std::numeric_limits<float>::infinity();
        if (o.colour && o.textures)
            // the colour image with the textured albedo: with or without the sampled emitters, with or without smooth normals
            check(trx_render_image_colour_textured(scene, &view, o.width, o.height, o.semantics, o.light_mask >= 0 ? (uint32_t)o.light_mask : 0u,
                                                   o.lights.empty() ? nullptr : o.lights.data(), (uint32_t)o.lights.size(), frame_count,
                                                   o.light_samples >= 0 ? (uint32_t)o.light_samples : 1u, o.shadow_eps >= 0.0f ? o.shadow_eps : 0.01f,
                                                   o.ambient >= 0.0f ? o.ambient : 0.1f, ao_samples, 0.0001f, radius,
                                                   o.ao_filter >= 0 ? (uint32_t)o.ao_filter : 0u, o.ao_depth_tol, o.ao_normal_cos,
                                                   o.bounce_samples >= 0 ? (uint32_t)o.bounce_samples : 0u, o.bounce_eps >= 0.0f ? o.bounce_eps : 0.01f,
                                                   o.bounce_filter >= 0 ? (uint32_t)o.bounce_filter : 0u, o.bounce_filter_tol, o.bounce_filter_cos,
                                                   o.bounce_stride >= 0 ? (uint32_t)o.bounce_stride : 1u, o.bounce_phase >= 0 ? (uint32_t)o.bounce_phase : 0u,
                                                   o.bounce_upsample >= 0 ? (uint32_t)o.bounce_upsample : 1u, o.emitters >= 0 ? (uint32_t)o.emitters : 0u,
                                                   o.emitter_eps >= 0.0f ? o.emitter_eps : 0.001f, o.smooth ? 1u : 0u, rgba.data(), &ms),
                  "png frame");
        else if (o.colour && o.emitters >= 0)
            // the colour image with the emissive triangles sampled as lights; there may be no --light at all
            check(trx_render_image_colour_emitters(scene, &view, o.width, o.height, o.semantics, o.light_mask >= 0 ? (uint32_t)o.light_mask : 0u,
                                                   o.lights.empty() ? nullptr : o.lights.data(), (uint32_t)o.lights.size(), frame_count,
                                                   o.light_samples >= 0 ? (uint32_t)o.light_samples : 1u, o.shadow_eps >= 0.0f ? o.shadow_eps : 0.01f,
                                                   o.ambient >= 0.0f ? o.ambient : 0.1f, ao_samples, 0.0001f, radius,
                                                   o.ao_filter >= 0 ? (uint32_t)o.ao_filter : 0u, o.ao_depth_tol, o.ao_normal_cos,
                                                   o.bounce_samples >= 0 ? (uint32_t)o.bounce_samples : 0u, o.bounce_eps >= 0.0f ? o.bounce_eps : 0.01f,
                                                   o.bounce_filter >= 0 ? (uint32_t)o.bounce_filter : 0u, o.bounce_filter_tol, o.bounce_filter_cos,
                                                   o.bounce_stride >= 0 ? (uint32_t)o.bounce_stride : 1u, o.bounce_phase >= 0 ? (uint32_t)o.bounce_phase : 0u,
                                                   o.bounce_upsample >= 0 ? (uint32_t)o.bounce_upsample : 1u, (uint32_t)o.emitters,
                                                   o.emitter_eps >= 0.0f ? o.emitter_eps : 0.001f, rgba.data(), &ms),
                  "png frame");
        else if (o.colour)
            // the colour image: the same chain, the bounce's term in three planes, composed with the scene's materials
            check((o.smooth ? trx_render_image_colour_smooth : trx_render_image_colour)(scene, &view, o.width, o.height, o.semantics, o.light_mask >= 0 ? (uint32_t)o.light_mask : 0u,
                                          o.lights.data(), (uint32_t)o.lights.size(), frame_count, o.light_samples >= 0 ? (uint32_t)o.light_samples : 1u,
                                          o.shadow_eps >= 0.0f ? o.shadow_eps : 0.01f, o.ambient >= 0.0f ? o.ambient : 0.1f, ao_samples, 0.0001f,
                                          radius, o.ao_filter >= 0 ? (uint32_t)o.ao_filter : 0u, o.ao_depth_tol, o.ao_normal_cos,
                                          o.bounce_samples >= 0 ? (uint32_t)o.bounce_samples : 0u, o.bounce_eps >= 0.0f ? o.bounce_eps : 0.01f,
                                          o.bounce_filter >= 0 ? (uint32_t)o.bounce_filter : 0u, o.bounce_filter_tol, o.bounce_filter_cos,
                                          o.bounce_stride >= 0 ? (uint32_t)o.bounce_stride : 1u, o.bounce_phase >= 0 ? (uint32_t)o.bounce_phase : 0u,
                                          o.bounce_upsample >= 0 ? (uint32_t)o.bounce_upsample : 1u, rgba.data(), &ms),
                  "png frame");
        else if (o.bounce_samples >= 0 && o.bounce_stride >= 0)
            // ... and one diffuse bounce traced at one pixel in stride x stride, upsampled (and filtered), on top of it
            check(trx_render_image_gi_sparse(scene, &view, o.width, o.height, o.semantics, o.light_mask >= 0 ? (uint32_t)o.light_mask : 0u,
                                             o.lights.data(), (uint32_t)o.lights.size(), frame_count, o.light_samples >= 0 ? (uint32_t)o.light_samples : 1u,
                                             o.shadow_eps >= 0.0f ? o.shadow_eps : 0.01f, o.ambient >= 0.0f ? o.ambient : 0.1f, ao_samples, 0.0001f,
                                             radius, o.ao_filter >= 0 ? (uint32_t)o.ao_filter : 0u, o.ao_depth_tol, o.ao_normal_cos,
                                             (uint32_t)o.bounce_samples, o.bounce_eps >= 0.0f ? o.bounce_eps : 0.01f,
                                             o.bounce_albedo >= 0.0f ? o.bounce_albedo : 0.5f, o.bounce_filter >= 0 ? (uint32_t)o.bounce_filter : 0u,
                                             o.bounce_filter_tol, o.bounce_filter_cos, (uint32_t)o.bounce_stride,
                                             o.bounce_phase >= 0 ? (uint32_t)o.bounce_phase : 0u, o.bounce_upsample >= 0 ? (uint32_t)o.bounce_upsample : 1u,
                                             rgba.data(), &ms),
                  "png frame");
        else if (o.bounce_samples >= 0 && o.bounce_filter >= 0)
            // ... and one diffuse bounce, filtered, on top of it
            check(trx_render_image_gi_filtered(scene, &view, o.width, o.height, o.semantics, o.light_mask >= 0 ? (uint32_t)o.light_mask : 0u,
                                               o.lights.data(), (uint32_t)o.lights.size(), frame_count, o.light_samples >= 0 ? (uint32_t)o.light_samples : 1u,
                                               o.shadow_eps >= 0.0f ? o.shadow_eps : 0.01f, o.ambient >= 0.0f ? o.ambient : 0.1f, ao_samples, 0.0001f,
                                               radius, o.ao_filter >= 0 ? (uint32_t)o.ao_filter : 0u, o.ao_depth_tol, o.ao_normal_cos,
                                               (uint32_t)o.bounce_samples, o.bounce_eps >= 0.0f ? o.bounce_eps : 0.01f,
                                               o.bounce_albedo >= 0.0f ? o.bounce_albedo : 0.5f, (uint32_t)o.bounce_filter, o.bounce_filter_tol,
                                               o.bounce_filter_cos, rgba.data(), &ms),
                  "png frame");
        else if (o.bounce_samples >= 0)
            // ... and one diffuse bounce on top of it (the GI image)
            check(trx_render_image_gi(scene, &view, o.width, o.height, o.semantics, o.light_mask >= 0 ? (uint32_t)o.light_mask : 0u,
                                      o.lights.data(), (uint32_t)o.lights.size(), frame_count, o.light_samples >= 0 ? (uint32_t)o.light_samples : 1u,
                                      o.shadow_eps >= 0.0f ? o.shadow_eps : 0.01f, o.ambient >= 0.0f ? o.ambient : 0.1f, ao_samples, 0.0001f,
                                      radius, o.ao_filter >= 0 ? (uint32_t)o.ao_filter : 0u, o.ao_depth_tol, o.ao_normal_cos,
                                      (uint32_t)o.bounce_samples, o.bounce_eps >= 0.0f ? o.bounce_eps : 0.01f,
                                      o.bounce_albedo >= 0.0f ? o.bounce_albedo : 0.5f, rgba.data(), &ms),
                  "png frame");
        else
            check((o.smooth ? trx_render_image_lit_smooth : trx_render_image_lit)(scene, &view, o.width, o.height, o.semantics, o.light_mask >= 0 ? (uint32_t)o.light_mask : 0u,
                                       o.lights.data(), (uint32_t)o.lights.size(), frame_count, o.light_samples >= 0 ? (uint32_t)o.light_samples : 1u,
                                       o.shadow_eps >= 0.0f ? o.shadow_eps : 0.01f, o.ambient >= 0.0f ? o.ambient : 0.1f, ao_samples, 0.0001f,
                                       radius, o.ao_filter >= 0 ? (uint32_t)o.ao_filter : 0u, o.ao_depth_tol, o.ao_normal_cos, rgba.data(), &ms),
                  "png frame");
        if (!write_png(path, rgba, o.width, o.height)) die("Failed to save image " + path);
        if (o.verbose) std::printf("saved %s (device image, %zu lights, %.3f ms)\n", path.c_str(), o.lights.size(), ms);
        return;
    }
    if (o.ao_samples != 0 || o.ao_radius > 0.0f) {
        // the AO term a renderer would use: the share of N bounded any-hit AO rays that reach nothing
        const unsigned samples = o.ao_samples ? o.ao_samples : 1u;
        const float radius = o.ao_radius > 0.0f ? o.ao_radius : std::numeric_limits<float>::infinity();
        if (o.ao_stride >= 0) {
            // the AO rays of one pixel in stride x stride, the term rebuilt and shaded on the device, 4 bytes per pixel back
            const uint32_t phase = o.ao_phase >= 0 ? (uint32_t)o.ao_phase : 0u, up = o.ao_upsample >= 0 ? (uint32_t)o.ao_upsample : 1u;
            check(trx_render_image_sparse(scene, &view, o.width, o.height, o.semantics, frame_count, samples, 0.0001f, radius,
                                          (uint32_t)o.ao_stride, phase, up, o.ao_depth_tol, o.ao_normal_cos, rgba.data(), &ms), "png frame");
            if (!write_png(path, rgba, o.width, o.height)) die("Failed to save image " + path);
            if (o.verbose)
                std::printf("saved %s (device image, AO stride %d phase %u, upsample radius %u, %.3f ms)\n", path.c_str(), o.ao_stride, phase, up, ms);
            return;
        }
        if (o.ao_filter >= 0) {
            // the image made on the device: filter and shade there, 4 bytes per pixel back
            check(trx_render_image(scene, &view, o.width, o.height, o.semantics, frame_count, samples, 0.0001f, radius,
                                   (uint32_t)o.ao_filter, o.ao_depth_tol, o.ao_normal_cos, rgba.data(), &ms), "png frame");
            if (!write_png(path, rgba, o.width, o.height)) die("Failed to save image " + path);
            if (o.verbose) std::printf("saved %s (device image, filter radius %d, %.3f ms)\n", path.c_str(), o.ao_filter, ms);
            return;
        }
        std::vector<uint8_t> counts(n);
        check(trx_trace_ao_visibility(scene, &view, o.width, o.height, o.semantics, frame_count, samples, 0.0001f, radius,
                                      counts.data(), &ms), "png frame");
        for (size_t i = 0; i < n; i++) {
            // (no surface: the reference's 1 / t of a miss, 0)
            const float col = counts[i] == TRX_AO_NO_SURFACE ? 0.0f : (float)counts[i] / (float)samples;
            const float g = std::pow(col, 2.2f) * 255.0f;
            rgba[4 * i + 0] = rgba[4 * i + 1] = rgba[4 * i + 2] = (unsigned char)(uint32_t)g;
            rgba[4 * i + 3] = 255;
        }
        if (!write_png(path, rgba, o.width, o.height)) die("Failed to save image " + path);
        if (o.verbose) std::printf("saved %s\n", path.c_str());
        return;
    }
    std::vector<trx_hit> primary(n), ao(n);
    check(trx_trace_primary_ao(scene, &view, o.width, o.height, o.semantics, frame_count, 0.0001f, primary.data(),
                               ao.data(), &ms), "png frame");
    for (size_t i = 0; i < n; i++) {
        float col = 1.0f / primary[i].t;
        if (primary[i].t < 3.4028234663852886e38f) col = ao[i].t < 3.4028234663852886e38f ? ao[i].t / (1.0f + ao[i].t) : 1.0f;
        const float g = std::pow(col, 2.2f) * 255.0f;
        const unsigned char c = (unsigned char)(uint32_t)(g < 0.f ? 0.f : g);
        rgba[4 * i + 0] = rgba[4 * i + 1] = rgba[4 * i + 2] = c;
        rgba[4 * i + 3] = 255;
    }
    if (!write_png(path, rgba, o.width, o.height)) die("Failed to save image " + path);
    if (o.verbose) std::printf("saved %s\n", path.c_str());
}

// one input of one pass: src/main.rs:241-478 (load, build, trace) -> Stats
Stats render_input(const Options &o, const std::string &input) {
    Stats st;
    float *verts = nullptr;
    uint64_t n_tris = 0, *counts = nullptr;
    uint32_t n_objects = 0;
    Camera cam;
    // --colour: the materials in the order of verts (permuted by tri_source once the scene is built)
    trx_material *materials = nullptr;
    uint32_t n_materials = 0;
    uint16_t *tri_material = nullptr;
    // --smooth: the vertex normals in the order of verts (permuted like the materials)
    float *normals = nullptr;
    uint32_t has_vn = 0;
    // --textures: the texcoords in the order of verts (permuted like the materials) and the texture set (keyed by material)
    std::vector<float> uvs;
    std::vector<trx_texture_desc> tex_descs;
    std::vector<uint32_t> texels, material_texture;
    const bool obj = input.size() > 4 && input.compare(input.size() - 4, 4, ".obj") == 0;
    if (input == "demoscene" || input.rfind("standin:", 0) == 0) {
        const std::string name = input == "demoscene" ? "demoscene" : input.substr(8);
        st.name = name;
        check(trx_gen_scene(name.c_str(), 0, 1, &verts, &n_tris, &counts, &n_objects), "scene");
        check(trx_scene_camera(name.c_str(), cam.eye, cam.look_at, &cam.fov), "camera");
        if (o.colour) check(trx_standin_materials(name.c_str(), verts, n_tris, counts, n_objects, &materials, &n_materials, &tri_material), "materials");
        if (o.textures) {
            uvs.resize((size_t)n_tris * 6);
            check(trx_standin_texcoords(name.c_str(), verts, n_tris, uvs.data()), "texcoords");
            trx_texture_desc *d = nullptr;
            uint32_t n_tex = 0, *tx = nullptr, *mt = nullptr;
            uint64_t n_texels = 0;
            check(trx_standin_textures(name.c_str(), n_materials, &d, &n_tex, &tx, &n_texels, &mt), "textures");
            tex_descs.assign(d, d + n_tex);
            texels.assign(tx, tx + n_texels);
            material_texture.assign(mt, mt + n_materials);
            trx_free(d);
            trx_free(tx);
            trx_free(mt);
        }
    } else if (obj) {
        // a model file on its own, with the materials of its mtl files: seen from +z, a box diagonal away from the box's centre
        size_t k = input.find_last_of('/');
        st.name = input.substr(k == std::string::npos ? 0 : k + 1);
        st.name.erase(st.name.size() - 4);
        check(trx_load_model_materials(input.c_str(), &verts, &n_tris, &counts, &n_objects, &materials, &n_materials, &tri_material), "model");
        if (o.smooth) { // (the same mesh again, byte for byte, with its `vn` records)
            float *v2 = nullptr;
            uint64_t n2 = 0, *c2 = nullptr;
            uint32_t o2 = 0;
            check(trx_load_model_normals(input.c_str(), &v2, &n2, &c2, &o2, &normals, &has_vn), "model normals");
            trx_free(v2);
            trx_free(c2);
            if (n2 != n_tris) die("model normals: the model changed while it was read");
        }
        if (o.textures) { // (the same mesh once more with its `vt` records; the map_Kd files from the OBJ's directory)
            float *v2 = nullptr, *uv = nullptr;
            uint64_t n2 = 0, *c2 = nullptr;
            uint32_t o2 = 0, has_vt = 0, n_names = 0;
            check(trx_load_model_texcoords(input.c_str(), &v2, &n2, &c2, &o2, &uv, &has_vt), "model texcoords");
            if (n2 != n_tris) die("model texcoords: the model changed while it was read");
            uvs.assign(uv, uv + (size_t)n_tris * 6);
            trx_free(v2);
            trx_free(c2);
            trx_free(uv);
            char *names = nullptr;
            check(trx_load_model_material_maps(input.c_str(), &names, &n_names), "material maps");
            if (n_names != n_materials) die("material maps: the model changed while it was read");
            const size_t slash = input.find_last_of('/');
            const std::string dir = slash == std::string::npos ? std::string() : input.substr(0, slash + 1);
            material_texture.assign(n_materials, TRX_NO_TEXTURE);
            const char *nm = names;
            for (uint32_t m = 0; m < n_materials; m++, nm += std::strlen(nm) + 1) {
                if (!*nm) continue;
                std::vector<uint32_t> px;
                uint32_t tw = 0, th = 0;
                if (!read_image(nm[0] == '/' ? std::string(nm) : dir + nm, px, tw, th)) continue;
                if (tex_descs.size() >= TRX_MAX_TEXTURES || texels.size() + px.size() >= 0x80000000ull) {
                    std::fprintf(stderr, "--textures: %s does not fit the texture set: its material stays untextured\n", nm);
                    continue;
                }
                material_texture[m] = (uint32_t)tex_descs.size();
                tex_descs.push_back(trx_texture_desc{tw, th, TRX_TEX_RGBA8_SRGB, TRX_TEX_BILINEAR});
                for (uint32_t y = 0; y < th; y++) // (image files are top-down: row 0 of a texture is the row at t = 0, the bottom one)
                    texels.insert(texels.end(), px.begin() + (size_t)(th - 1 - y) * tw, px.begin() + (size_t)(th - y) * tw);
            }
            trx_free(names);
            if (!has_vt) std::fprintf(stderr, "--textures: %s has no usable vt: every corner gets 0, 0\n", input.c_str());
        }
        float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
        for (uint64_t i = 0; i < n_tris * 3; i++)
            for (int c = 0; c < 3; c++) {
                const float x = verts[i * 3 + c];
                if (i == 0 || x < lo[c]) lo[c] = x;
                if (i == 0 || x > hi[c]) hi[c] = x;
            }
        float diag = 0;
        for (int c = 0; c < 3; c++) {
            cam.look_at[c] = cam.eye[c] = 0.5f * (lo[c] + hi[c]);
            diag += (hi[c] - lo[c]) * (hi[c] - lo[c]);
        }
        cam.eye[2] += std::sqrt(diag) > 0.0f ? std::sqrt(diag) : 1.0f;
        cam.fov = 60.0f;
    } else {
        if (o.colour) die("--colour takes the materials of -i <file.obj> or of standin:<name>");
        size_t k = input.find_last_of('/');
        st.name = input.substr(k == std::string::npos ? 0 : k + 1);
        k = st.name.find_last_of('.');
        if (k != std::string::npos) st.name.erase(k);
        // scene file + model through the library's loader (src/main.rs:259-298: "Failed to load config" / the model's error)
        check(trx_load_scene(input.c_str(), &verts, &n_tris, &counts, &n_objects, cam.eye, cam.look_at, &cam.fov), "scene");
    }
    if (o.smooth && !has_vn) { // no usable `vn` (always so for a generated scene): computed from the mesh
        trx_free(normals);
        normals = static_cast<float *>(std::malloc(std::max<size_t>((size_t)n_tris * 9 * sizeof(float), 4)));
        if (!normals) die("out of memory");
        const double deg = o.smooth_crease >= 0.0f ? (double)o.smooth_crease : 45.0;
        check(trx_compute_vertex_normals(verts, n_tris, (float)std::cos(deg * 3.14159265358979323846 / 180.0), normals), "vertex normals");
    }
    const bool tlas = o.tlas && !o.flatten_blas; // src/main.rs:300-308
    if (o.verbose) std::printf("%u objects \"%s\"\ntriangles %llu\n", n_objects, st.name.c_str(), (unsigned long long)n_tris);
    trx_flat *flat = nullptr;
    check(trx_set_build_device(o.gpu_build ? o.device : -1), "build device");
    if (o.preset.empty()) {
        // no preset: BvhBuildParams from the individual flags (src/main.rs:571-585), the ploc_cwbvh pipeline
        trx_build_params bp;
        trx_build_params_default(&bp);
        bp.pre_split = o.split ? 1u : 0u;
        bp.ploc_search_distance = o.search_distance;
        bp.search_depth_threshold = o.search_depth_threshold;
        bp.reinsertion_batch_ratio = o.reinsertion_batch_ratio;
        bp.sort_precision = o.sort_precision;
        bp.max_prims_per_leaf = o.max_prims_per_leaf;
        bp.post_collapse_reinsertion_batch_ratio_multiplier = o.post_collapse_multiplier;
        bp.collapse_traversal_cost = o.collapse_traversal_cost;
        check(trx_flat_build_params(verts, counts, n_objects, tlas ? 1 : 0, &bp, 0, &flat), "build");
    } else {
        // a named preset overrides the individual builder flags (src/main.rs:563-570); obvhs' preset values are not in
        // the reference tree, so the names select this library's own settings of matching cost
        check(trx_set_build_costs(o.collapse_traversal_cost, 0.3f), "build costs");
        check(trx_set_build_preset(o.preset.c_str()), "preset");
        if (o.gpu_build) // every stage of the preset's build on the device (PLOC + whole-iteration reinsertion + collapse)
            check(trx_flat_build_preset_device(verts, counts, n_objects, tlas ? 1 : 0, o.preset.c_str(), o.max_prims_per_leaf, 0, o.device,
                                               &flat), "build");
        else
            check(trx_flat_build(verts, counts, n_objects, tlas ? 1 : 0, o.max_prims_per_leaf, 0, &flat), "build");
    }
    st.blas_build_time_s = flat->blas_build_s;
    st.tlas_build_time_ms = flat->tlas_build_s * 1000.0;
    if (o.verbose) std::printf("nodes %llu tlas_start %u instances %u\n", (unsigned long long)flat->n_nodes, flat->tlas_start, flat->n_instances);
    if (o.dry_run) { // scene file, model and build only: nothing below this line works without a device
        if (o.verbose) std::printf("camera eye %g %g %g look_at %g %g %g fov %g\n", cam.eye[0], cam.eye[1], cam.eye[2],
                                   cam.look_at[0], cam.look_at[1], cam.look_at[2], cam.fov);
        trx_flat_destroy(flat);
        trx_free(verts);
        trx_free(counts);
        trx_free(materials);
        trx_free(tri_material);
        trx_free(normals);
        return st;
    }

    trx_scene *scene = nullptr;
    check(trx_scene_create(flat->bvh_bytes, flat->n_nodes, flat->tri_verts, flat->n_tris, TRX_TRI_VERTS_36,
                           flat->n_instances ? flat->instance_offsets : nullptr, flat->n_instances, flat->tlas_start,
                           o.device, &scene), "scene upload");
    // a re-braided TLAS (trx_set_build_rebraid, on by default) names the node of its BLAS at which each primitive's walk
    // starts; without the table every primitive would enter its BLAS at the root and a ray crossing k sub-boxes of one
    // BLAS would walk that BLAS k times (same hits, many more node visits)
    if (flat->instance_entry_nodes && flat->n_instances)
        check(trx_scene_set_instance_entry_nodes(scene, flat->instance_entry_nodes, flat->n_instances), "instance entry nodes");
    if (o.colour) { // the table in `prim` order: record i of the scene is triangle tri_source[i] of the mesh
        std::vector<uint16_t> by_prim(flat->n_tris);
        for (uint64_t i = 0; i < flat->n_tris; i++) by_prim[i] = flat->tri_source[i] < n_tris ? tri_material[flat->tri_source[i]] : 0;
        check(trx_scene_set_materials(scene, materials, n_materials, by_prim.data(), flat->n_tris), "materials");
    }
    if (o.smooth) { // the normals in `prim` order, like the materials
        std::vector<float> by_prim((size_t)flat->n_tris * 9, 0.0f);
        for (uint64_t i = 0; i < flat->n_tris; i++)
            if (flat->tri_source[i] < n_tris) std::memcpy(&by_prim[i * 9], normals + (size_t)flat->tri_source[i] * 9, 9 * sizeof(float));
        check(trx_scene_set_vertex_normals(scene, by_prim.data(), flat->n_tris), "vertex normals");
    }
    if (o.textures) { // the texcoords in `prim` order, like the materials; the texture set where any image was read
        std::vector<float> by_prim((size_t)flat->n_tris * 6, 0.0f);
        for (uint64_t i = 0; i < flat->n_tris; i++)
            if (flat->tri_source[i] < n_tris) std::memcpy(&by_prim[i * 6], &uvs[(size_t)flat->tri_source[i] * 6], 6 * sizeof(float));
        check(trx_scene_set_texcoords(scene, by_prim.data(), flat->n_tris), "texcoords");
        if (!tex_descs.empty())
            check(trx_scene_set_textures(scene, tex_descs.data(), (uint32_t)tex_descs.size(), texels.data(), texels.size(), material_texture.data(),
                                         n_materials), "textures");
    }
    trx_view view;
    check(trx_view_from_camera(cam.eye, cam.look_at, cam.fov, (float)o.width, (float)o.height, &view), "camera");

    // frames until render_time is used up; --benchmark adds the untimed warm-up dispatch and the result
    // is the MINIMUM frame time (src/rt_gpu/rt_gpu_software.rs:289-302,339,376)
    double total_ms = 0, min_ms = 1e30;
    unsigned frames = 0, frame_count = 0;
    if (o.overlap) {
        // The same loop without the host between its frames, and with frame i's AO pass on a second stream under frame
        // i + 1's primary pass: batches of frames until render_time is used up.  A frame has no time of its own here, so the
        // result is the average over the last batch (with --benchmark: the best batch's average).
        unsigned batch = 16;
        float ms = 0;
        if (o.benchmark) check(trx_frame_loop(scene, &view, o.width, o.height, o.semantics, 0, 0, 0.0001f, 8, 1, nullptr, nullptr, &ms), "warm-up");
        do {
            check(trx_frame_loop(scene, &view, o.width, o.height, o.semantics, frame_count, o.animate ? 1 : 0, 0.0001f, batch, 1, nullptr,
                                 nullptr, &ms), "trace");
            total_ms += ms;
            min_ms = std::min(min_ms, (double)ms / batch);
            frames += batch;
            if (o.animate) frame_count = frames;
        } while (total_ms < o.render_time * 1000.0 && frames < 100000);
    } else {
        if (o.benchmark) {
            float ms = 0;
            check(trx_trace_primary_ao(scene, &view, o.width, o.height, o.semantics, 0, 0.0001f, nullptr, nullptr, &ms), "warm-up");
        }
        do {
            float ms = 0;
            check(trx_trace_primary_ao(scene, &view, o.width, o.height, o.semantics, frame_count, 0.0001f, nullptr, nullptr, &ms),
                  "trace");
            total_ms += ms;
            min_ms = std::min(min_ms, (double)ms);
            frames++;
            if (o.animate) frame_count = frames;
        } while (total_ms < o.render_time * 1000.0 && frames < 100000);
    }
    st.traversal_ms = o.benchmark ? min_ms : total_ms / frames;
    if (o.verbose) std::printf("%.2fms   avg render time over %u frames (min %.3fms)\n", total_ms / frames, frames, min_ms);
    if (o.png) save_png(o, scene, view, frame_count, st.name);

    trx_scene_destroy(scene);
    trx_flat_destroy(flat);
    trx_free(verts);
    trx_free(counts);
    trx_free(materials);
    trx_free(tri_material);
    trx_free(normals);
    return st;
}

void print_table(const std::vector<Stats> &rows) { // tabled Style::blank(), src/main.rs:207,634-640
    const char *hdr[4] = {"name", "traversal_ms", "blas_build_time_s", "tlas_build_time_ms"};
    std::vector<std::vector<std::string>> cells;
    for (const Stats &s : rows) {
        char a[64], b[64], c[64];
        std::snprintf(a, sizeof(a), "%g", s.traversal_ms);
        std::snprintf(b, sizeof(b), "%g", s.blas_build_time_s);
        std::snprintf(c, sizeof(c), "%g", s.tlas_build_time_ms);
        cells.push_back({s.name, a, b, c});
    }
    size_t wdt[4];
    for (int k = 0; k < 4; k++) {
        wdt[k] = std::strlen(hdr[k]);
        for (auto &r : cells) wdt[k] = std::max(wdt[k], r[k].size());
    }
    for (int k = 0; k < 4; k++) std::printf(" %-*s ", (int)wdt[k], hdr[k]);
    std::printf("\n");
    for (auto &r : cells) {
        for (int k = 0; k < 4; k++) std::printf(" %-*s ", (int)wdt[k], r[k].c_str());
        std::printf("\n");
    }
}

} // namespace

int main(int argc, char **argv) {
    Options o = parse_args(argc, argv);
    if (!o.dry_run && trx_device_count() <= o.device) die("no HIP device " + std::to_string(o.device) + " (libtrx.so has no CPU fallback)");
    std::vector<std::string> inputs;
    {
        std::stringstream ss(o.input);
        std::string item;
        while (std::getline(ss, item, ',')) if (!item.empty()) inputs.push_back(item);
    }
    std::vector<Stats> avg;
    for (unsigned pass = 0; pass < o.passes; pass++) {
        std::vector<Stats> stats;
        for (const std::string &in : inputs) stats.push_back(render_input(o, in));
        Stats a; // the "Avg" row, src/main.rs:479-488
        a.name = "Avg";
        for (const Stats &s : stats) {
            a.traversal_ms += s.traversal_ms / stats.size();
            a.blas_build_time_s += s.blas_build_time_s / stats.size();
            a.tlas_build_time_ms += s.tlas_build_time_ms / stats.size();
        }
        stats.push_back(a);
        if (avg.empty()) {
            avg = stats;
            for (Stats &s : avg) s.traversal_ms = s.blas_build_time_s = s.tlas_build_time_ms = 0;
        }
        for (size_t i = 0; i < stats.size(); i++) { // averaged over passes, src/main.rs:191-206
            avg[i].traversal_ms += stats[i].traversal_ms / o.passes;
            avg[i].blas_build_time_s += stats[i].blas_build_time_s / o.passes;
            avg[i].tlas_build_time_ms += stats[i].tlas_build_time_ms / o.passes;
        }
    }
    print_table(avg);
    return 0;
}
