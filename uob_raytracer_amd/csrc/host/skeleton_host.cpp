// skeleton_host.cpp — the reference's application loop (Source/skeleton.cpp:93-144) over libuob_rt.so.
//
// Same globals and function names as the reference: focal_length, camera_position, yaw, pitch,
// light_position (skeleton.cpp:61-67), update() (:282-361), draw via offload_rendering() (:146-182),
// opencl_initialise() (:366-497) — the last two now four lines each over the C ABI.
// SDL events do not exist headless: update() keeps the light animation (:290-298) bit for bit and takes its events from
// an optional script that stands for SDL's event queue: key names ("up down left right i o k j esc", :311-352), mouse
// motion "m:dx,dy" (SDL_MOUSEMOTION xrel / yrel, :306-309) and "." (the queue is empty for the rest of this frame).
// As in the reference's polling loop a frame consumes mouse events until it meets a key (handled, then update()
// returns: what is left waits for the next frame), a "." or the end of the script.
//
//   uob_raytracer [--size N] [--frames K] [--aa X Y] [--shadows S] [--keys "left m:12,-3 . left i"] [--out file.bmp]
//                 [--obj mesh.obj]            append load_obj(mesh.obj) to the box, as skeleton.cpp:102-103 does
//                 [--move DX,DY,DZ]           with --obj: update() slides the mesh by (DX,DY,DZ) every frame (float32
//                                             adds to its vertices; normals do not change), rt_update_scene before the frame
//                 [--spin RAD]                with --obj: the mesh is one rigid object (rt_set_objects); frame f = 1, 2, ... poses
//                                             it by a rotation of f * RAD about the vertical axis through the centre of
//                                             its rest bounding box (rt_pose_objects: 48 bytes per frame cross the bus)
//                 [--bend RAD]                with --obj: the mesh is skinned to two bones (rt_set_skin), bone 1 weighted by
//                                             (y - ymin) / (ymax - ymin) of the rest vertex and bone 0 by the rest; frame
//                                             f = 1, 2, ... keeps bone 0 and turns bone 1 by f * RAD about the vertical axis
//                                             through the centre of the rest mesh's bounding box, as --spin turns the
//                                             mesh (rt_pose_skin: 96 bytes per frame cross the bus)
//                 [--bounce-sphere]           sphere 0 follows a parabola, frame by frame (rt_update_spheres)
//                 [--gpus N | --devices a,b,..]  render every frame on several GPUs inside the one context
//                 [--copy-back]                  device buffer + blocking read-back instead of rt_register_output
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../../include/uob_rt.h"
#include "screen.h"

using namespace std;
using namespace std::chrono;

int SCREEN_WIDTH = 1024, SCREEN_HEIGHT = 1024;                 // skeleton.cpp:32-33

float focal_length = 2200.0;                                   // :61
float camera_position[4] = {0.0f, 0.0f, -3.2f, 1.0f};          // :62 (glm::vec4)
float pitch = 0.0f, yaw = 0.0f;                                // :65-66
float light_position[4] = {0.0f, -0.5f, -0.7f, 1.0f};          // :67
bool quit = false;
bool lor = true;                                               // :74
vector<rt_triangle> triangles;                                 // :72
static rt_ctx* g_rt = nullptr;
static vector<string> g_keys;                                  // scripted key presses, one per frame
static size_t g_key_at = 0;
static size_t g_obj_first = 0;                                 // --move: the loaded mesh is triangles[g_obj_first..]
static bool g_move = false;
static float g_move_by[3] = {0.0f, 0.0f, 0.0f};
static bool g_spin = false;                                    // --spin: the loaded mesh turns as one rigid object
static float g_turn_rad = 0.0f;                               // --spin / --bend: the angle per frame
static float g_turn_centre[3] = {0.0f, 0.0f, 0.0f};            // centre of the rest mesh's bounding box
static bool g_bend = false;                                    // --bend: the loaded mesh bends between two bones
static bool g_bounce = false;                                  // --bounce-sphere: sphere 0 follows a parabola, frame by frame
static rt_sphere g_spheres[RT_MAX_SPHERES];
static int g_num_spheres = 0;

static void die(const char* op) {                              // checkError(), :499-507
  fprintf(stderr, "Error during operation '%s': %s\n", op, rt_last_error());
  exit(EXIT_FAILURE);
}

void opencl_initialise(const rt_config& cfg) {                 // :366-497
  const int n = (int)triangles.size();
  vector<float> v(12 * (size_t)n), nr(4 * (size_t)n), col(4 * (size_t)n);
  rt_scene_pack(triangles.data(), n, v.data(), nr.data(), col.data());     // :474-484
  if (rt_init(&cfg, v.data(), nr.data(), col.data(), n, &g_rt) != RT_OK) die("rt_init");
}

// The moved scene to the device before the frame: the scene is no longer fixed after opencl_initialise
void update_scene() {
  const int n = (int)triangles.size();
  vector<float> v(12 * (size_t)n), nr(4 * (size_t)n), col(4 * (size_t)n);
  rt_scene_pack(triangles.data(), n, v.data(), nr.data(), col.data());
  if (rt_update_scene(g_rt, v.data(), nr.data(), col.data(), n, 0) != RT_OK) die("rt_update_scene");
}

// The bounding box of the loaded mesh as it stands, and its centre into g_turn_centre
static void mesh_box(float lo[3], float hi[3]) {
  for (int k = 0; k < 3; ++k) lo[k] = hi[k] = triangles[g_obj_first].v0[k];
  for (size_t t = g_obj_first; t < triangles.size(); ++t)
    for (const float* p : {triangles[t].v0, triangles[t].v1, triangles[t].v2})
      for (int k = 0; k < 3; ++k) { if (p[k] < lo[k]) lo[k] = p[k]; if (p[k] > hi[k]) hi[k] = p[k]; }
  for (int k = 0; k < 3; ++k) g_turn_centre[k] = (lo[k] + hi[k]) * 0.5f;
}

// The mesh becomes the context's one object; its rest pose is the scene as uploaded
void spin_begin() {
  float lo[3], hi[3];
  mesh_box(lo, hi);
  const int32_t first = (int32_t)g_obj_first, count = (int32_t)(triangles.size() - g_obj_first);
  if (rt_set_objects(g_rt, &first, &count, 1) != RT_OK) die("rt_set_objects");
}

// The rest pose turned by f * RAD about the vertical axis through the centre c: v' = M v + (c - M c), M as
// rt_rotation_matrix builds it (float cos / sin)
static void turn_about_centre(int f, float x[12]) {
  rt_rotation_matrix((float)f * g_turn_rad, 0.0f, x);
  const float* c = g_turn_centre;
  for (int r = 0; r < 3; ++r) x[4 * r + 3] = c[r] - ((c[0] * x[4 * r] + c[1] * x[4 * r + 1]) + c[2] * x[4 * r + 2]);
}

// The mesh of frame f = 1, 2, ...: turned as one rigid object; to the device before the frame
void spin_mesh(int f) {
  float x[12];
  turn_about_centre(f, x);
  if (rt_pose_objects(g_rt, x, 0) != RT_OK) die("rt_pose_objects");
}

// The mesh is skinned to two bones by the height of its rest vertices: bone 1 weighs (y - ymin) / (ymax - ymin), clamped to
// [0, 1], bone 0 the rest; its rest pose is the scene as uploaded
void bend_begin() {
  float lo[3], hi[3];
  mesh_box(lo, hi);
  const size_t count = triangles.size() - g_obj_first;
  vector<uint16_t> index(12 * count, 0);
  vector<float> weights(12 * count, 0.0f);
  const float height = hi[1] - lo[1];
  size_t corner = 0;
  for (size_t t = g_obj_first; t < triangles.size(); ++t)
    for (const float* p : {triangles[t].v0, triangles[t].v1, triangles[t].v2}) {
      float w = height > 0.0f ? (p[1] - lo[1]) / height : 0.0f;
      w = w < 0.0f ? 0.0f : (w > 1.0f ? 1.0f : w);
      index[4 * corner + 1] = 1;
      weights[4 * corner] = 1.0f - w; weights[4 * corner + 1] = w;
      ++corner;
    }
  if (rt_set_skin(g_rt, (int32_t)g_obj_first, (int32_t)count, index.data(), weights.data(), 2) != RT_OK) die("rt_set_skin");
}

// The mesh of frame f = 1, 2, ...: bone 0 stays, bone 1 turns as --spin turns the mesh; to the device before the frame
void bend_mesh(int f) {
  float bones[24] = {1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f};
  turn_about_centre(f, bones + 12);
  if (rt_pose_skin(g_rt, bones, 0) != RT_OK) die("rt_pose_skin");
}

// Sphere 0 of frame f = 1, 2, ... on a fixed parabola (one bounce in eight frames), to the device before the frame
void bounce_sphere(int f) {
  const float u = (float)(f % 8) * 0.125f;
  g_spheres[0].center[0] = 0.3f - u * 0.25f;
  g_spheres[0].center[1] = 0.1f - (u * (1.0f - u)) * 0.8f;
  if (rt_update_spheres(g_rt, g_spheres, g_num_spheres) != RT_OK) die("rt_update_spheres");
}

void offload_rendering(screen* screen) {                       // :146-182
  float rot[12];
  rt_rotation_matrix(yaw, pitch, rot);                         // :149-151
  if (rt_render(g_rt, rot, camera_position, light_position, focal_length, screen->buffer, nullptr) != RT_OK)
    die("rt_render");
}

bool update() {                                                // :282-361
  if (lor) {                                                   // light oscillation, :290-298
    float diff = -0.5f - light_position[0];
    if (diff > -0.001f) lor = false;
    light_position[0] += diff / 20.0f;
  } else {
    float diff = 0.5f - light_position[0];
    if (diff < 0.001f) lor = true;
    light_position[0] += diff / 20.0f;
  }
  if (g_move)                                                  // the moving object: a translation of the loaded mesh
    for (size_t t = g_obj_first; t < triangles.size(); ++t)
      for (float* p : {triangles[t].v0, triangles[t].v1, triangles[t].v2})
        for (int k = 0; k < 3; ++k) p[k] += g_move_by[k];
  while (g_key_at < g_keys.size()) {                           // while(SDL_PollEvent(&e)), :300-301
    const string& k = g_keys[g_key_at++];
    if (k == ".") return false;                                // no more events this frame
    if (k.compare(0, 2, "m:") == 0) {                          // SDL_MOUSEMOTION, :306-309
      int xrel = 0, yrel = 0;
      if (sscanf(k.c_str() + 2, "%d,%d", &xrel, &yrel) != 2) { fprintf(stderr, "bad mouse event '%s' (m:dx,dy)\n", k.c_str()); exit(2); }
      yaw += xrel * 0.0009f;
      pitch -= yrel * 0.0009f;
      continue;
    }
    if (k == "up") pitch -= 0.1;
    else if (k == "down") pitch += 0.1;
    else if (k == "left") yaw += 0.1;
    else if (k == "right") yaw -= 0.1;
    else if (k == "i") camera_position[2] += 0.1;
    else if (k == "o") camera_position[2] -= 0.1;
    else if (k == "k") camera_position[0] += 0.1;
    else if (k == "j") camera_position[0] -= 0.1;
    else if (k == "esc") { quit = true; return false; }
    return true;
  }
  return false;
}

int main(int argc, char* argv[]) {
  bool direct_out = true;
  int frames = 10;
  const char* out = "screenshot.bmp";
  const char* obj = nullptr;
  const char* aov = nullptr;
  rt_config cfg;
  rt_config_default(&cfg);
  for (int i = 1; i < argc; ++i) {
    string a = argv[i];
    if (a == "--size" && i + 1 < argc) SCREEN_WIDTH = SCREEN_HEIGHT = atoi(argv[++i]);
    else if (a == "--frames" && i + 1 < argc) frames = atoi(argv[++i]);
    else if (a == "--aa" && i + 2 < argc) { cfg.aa_x = atoi(argv[++i]); cfg.aa_y = atoi(argv[++i]); }
    else if (a == "--shadows" && i + 1 < argc) cfg.shadow_samples = atoi(argv[++i]);
    else if (a == "--keys" && i + 1 < argc) { istringstream in(argv[++i]); string k; while (in >> k) g_keys.push_back(k); }
    else if (a == "--out" && i + 1 < argc) out = argv[++i];
    else if (a == "--obj" && i + 1 < argc) obj = argv[++i];
    else if (a == "--aov" && i + 1 < argc) aov = argv[++i];       // PREFIX of the last view's depth / normal / id images
    else if (a == "--move" && i + 1 < argc) {
      if (sscanf(argv[++i], "%f,%f,%f", &g_move_by[0], &g_move_by[1], &g_move_by[2]) != 3) { fprintf(stderr, "--move DX,DY,DZ\n"); return 2; }
      g_move = true;
    }
    else if (a == "--spin" && i + 1 < argc) { g_turn_rad = (float)atof(argv[++i]); g_spin = true; }
    else if (a == "--bend" && i + 1 < argc) { g_turn_rad = (float)atof(argv[++i]); g_bend = true; }
    else if (a == "--bounce-sphere") g_bounce = true;
    else if (a == "--copy-back") direct_out = false;           // render into device memory + blocking copy, as the reference reads back
    else if (a == "--gpus" && i + 1 < argc) {
      cfg.num_devices = atoi(argv[++i]);
      if (cfg.num_devices < 1 || cfg.num_devices > RT_MAX_DEVICES) { fprintf(stderr, "--gpus must be in [1,%d]\n", RT_MAX_DEVICES); return 2; }
      for (int d = 0; d < cfg.num_devices; ++d) cfg.devices[d] = d;
    } else if (a == "--devices" && i + 1 < argc) {
      istringstream in(argv[++i]); string tok; cfg.num_devices = 0;
      while (getline(in, tok, ',') && cfg.num_devices < RT_MAX_DEVICES) cfg.devices[cfg.num_devices++] = atoi(tok.c_str());
    }
    else { fprintf(stderr, "unknown argument %s\n", a.c_str()); return 2; }
  }
  cfg.width = SCREEN_WIDTH; cfg.height = SCREEN_HEIGHT; cfg.band_rows = SCREEN_HEIGHT;
  focal_length = 1100.0f * (float)SCREEN_WIDTH / 1024.0f * (float)cfg.aa_x;   // 2200 at the reference's 1024 / 2x2

  screen* screen = InitializeSDL(SCREEN_WIDTH, SCREEN_HEIGHT, false);         // :98
  triangles.resize(64);
  const int n = rt_scene_cornell_box(triangles.data(), 64);                   // LoadTestModel, :101
  if (n < 0) die("rt_scene_cornell_box");
  triangles.resize(n);
  g_obj_first = triangles.size();
  if (g_move && !obj) { fprintf(stderr, "--move needs --obj\n"); return 2; }
  if (g_spin && !obj) { fprintf(stderr, "--spin needs --obj\n"); return 2; }
  if (g_spin && g_move) { fprintf(stderr, "--spin and --move exclude each other (--move replaces the scene behind the rest pose)\n"); return 2; }
  if (g_bend && !obj) { fprintf(stderr, "--bend needs --obj\n"); return 2; }
  if (g_bend && (g_spin || g_move)) { fprintf(stderr, "--bend excludes --spin and --move (one rest pose, one table)\n"); return 2; }
  g_num_spheres = cfg.num_spheres;
  for (int i = 0; i < RT_MAX_SPHERES; ++i) g_spheres[i] = cfg.spheres[i];
  if (obj) {                                                                   // load_obj + insert, :102-103
    const int m = rt_scene_load_obj(obj, nullptr, 0);
    if (m < 0) die("rt_scene_load_obj");
    triangles.resize((size_t)n + m);
    if (rt_scene_load_obj(obj, triangles.data() + n, m) != m) die("rt_scene_load_obj");
  }
  printf("Triangles Length size %lu\n", triangles.size());                    // :104
  opencl_initialise(cfg);                                                      // :106
  if (g_spin && triangles.size() > g_obj_first) spin_begin();
  if (g_bend && triangles.size() > g_obj_first) bend_begin();
  // the device(s) write finished pixels straight into screen->buffer (no read-back after the kernel)
  if (direct_out &&
      rt_register_output(g_rt, screen->buffer, (size_t)SCREEN_WIDTH * SCREEN_HEIGHT * sizeof(uint32_t)) != RT_OK)
    die("rt_register_output");

  offload_rendering(screen);                                                   // initial scene, :109-110
  SDL_Renderframe(screen);
  for (int f = 0; f < frames && !quit; ++f) {                                  // :117-138
    update();
    if (g_move) update_scene();
    if (g_spin && triangles.size() > g_obj_first) spin_mesh(f + 1);
    if (g_bend && triangles.size() > g_obj_first) bend_mesh(f + 1);
    if (g_bounce) bounce_sphere(f + 1);
    auto start = high_resolution_clock::now();
    offload_rendering(screen);
    auto stop = high_resolution_clock::now();
    auto offload_duration = duration_cast<microseconds>(stop - start);
    cout << "\nOffloaded GPU Rendertime: " << offload_duration.count() << " micro seconds" << endl;
    cout << "Frame Rate: " << 1000000.0f / ((float)offload_duration.count()) << "FPS" << endl;
    SDL_Renderframe(screen);
  }
  SDL_SaveImage(screen, out);                                                  // :139
  if (aov) {                                                                   // what the last frame's pixels see (sample 0)
    const size_t px = (size_t)SCREEN_WIDTH * SCREEN_HEIGHT;
    vector<int32_t> prim(px);
    vector<float> depth(px), normal(4 * px);
    float rot[12];
    rt_rotation_matrix(yaw, pitch, rot);
    rt_aov_buffers planes;
    memset(&planes, 0, sizeof planes);
    planes.prim = prim.data(); planes.depth = depth.data(); planes.normal4 = normal.data();
    if (rt_render_aov(g_rt, rot, camera_position, focal_length, 0, &planes) != RT_OK) die("rt_render_aov");
    SaveAovImages(aov, SCREEN_WIDTH, SCREEN_HEIGHT, prim.data(), depth.data(), normal.data());
  }
  printf("light_position.x %.9g yaw %.9g pitch %.9g camera %.9g %.9g\n", light_position[0], yaw, pitch,
         camera_position[0], camera_position[2]);
  rt_destroy(g_rt);
  KillSDL(screen);
  return 0;
}
