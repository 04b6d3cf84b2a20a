// scenes.h — procedural stand-in scenes and model loading (see scenes.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace trx {

bool gen_scene(const std::string &name, uint64_t n_tris, uint64_t seed, std::vector<float> &verts,
               std::vector<uint64_t> &objects);
bool scene_camera(const std::string &name, float eye[3], float look_at[3], float *fov_deg);
bool load_model(const std::string &path, std::vector<float> &verts, std::vector<uint64_t> &objects);
// load_model with the model's materials (trx_load_model_materials): the same verts and objects, a table of 6 floats per
// material (albedo, emission; material 0 the default 0.8 / 0, then the mtl files' newmtl entries in file order) and one index
// per triangle in the order of verts.  false with `error` set: a mtl file the loader refuses; false without: unreadable.
struct ModelMaterials {
    std::vector<float> table;
    std::vector<uint16_t> tri;
    std::string error;
};
bool load_model_materials(const std::string &path, std::vector<float> &verts, std::vector<uint64_t> &objects, ModelMaterials &mm);
// load_model with the model's vertex normals (trx_load_model_normals): the same verts and objects, nine floats per triangle
// in the order of verts (an OBJ corner's `vn`, +0 where it names none or one out of range; all +0 for a JSON model) and
// whether any corner got one.  false with `error` set: a `vn` the loader refuses; false without: unreadable.
struct ModelNormals {
    std::vector<float> normals;
    bool any = false;
    std::string error;
};
bool load_model_normals(const std::string &path, std::vector<float> &verts, std::vector<uint64_t> &objects, ModelNormals &mn);
// load_model with the model's texture coordinates (trx_load_model_texcoords): the same verts and objects, six floats per
// triangle in the order of verts (an OBJ corner's `vt`, +0, +0 where it names none or one out of range; all +0 for a JSON
// model) and whether any corner got one.  false: unreadable.
struct ModelTexcoords {
    std::vector<float> uvs;
    bool any = false;
};
bool load_model_texcoords(const std::string &path, std::vector<float> &verts, std::vector<uint64_t> &objects, ModelTexcoords &mt);
// The `map_Kd` file name of every material of load_model_materials' table, in its order (trx_load_model_material_maps): an empty
// string where a material names none; material 0 never does.  false with `error` set: a mtl file the loader refuses.
bool load_model_material_maps(const std::string &path, std::vector<std::string> &maps, std::string &error);
// Vertex normals from the mesh alone (include/trx.h, trx_compute_vertex_normals): nine floats per triangle into out.
void compute_vertex_normals(const float *verts, uint64_t n_tris, double crease_cos, float *out);
// A scene file of the reference (assets/scenes/*.ron: model_path, camera(eye, look_at, fov)): the model's path resolved by
// the reference's rule (src/main.rs:271-284) and the camera.  false = unreadable or not such a file.
bool parse_scene_ron(const std::string &path, std::string &model_path, float eye[3], float look_at[3], float *fov_deg);

} // namespace trx
