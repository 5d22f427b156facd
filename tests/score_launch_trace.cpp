// Stand-alone host program for tests/test_scoring_plan.py: loads libvad_hip.so and digests what the four scoring entry points
// (vad_img_score_c, vad_vid_score_s, vad_vid_score_windows_c, vad_convlstm_seq) WOULD do - every kernel launch with its symbol,
// grid, block, dynamic LDS, stream and the offset from the workspace base of every kernel-parameter word that points into the
// workspace; every event record and stream wait - by defining the HIP entry points those paths use itself.  Nothing reaches a
// GPU, none is needed.  The workspace is an address range of exactly the reported size that is never dereferenced, every other
// pointer a distinct made-up address.  Part of what the digests record: the device-properties query fails (the library then
// assumes 256 CUs) and the occupancy query answers 2.
// usage: score_launch_trace <libvad_hip.so> <symbols: "hex-offset name" per line> <script> [dump]
// script lines:  group <name> | set <vad_debug_set_* symbol> <int>
//                img <fmt> <prec> <in_ch> <b> <h> <w> <latent> <chunk> <outputs: bit 0 scores, 1 errmap, 2 recon, 3 latent>
//                vid <fmt> <prec> <in_ch> <b> <t> <h> <w> <latent> <hid> <layers> <chunk> <outputs: 0 seq, 1 frame, 2 errmap, 3 recon, 4 state_in, 5 state_out>
//                win <fmt> <prec> <in_ch> <frames> <t> <stride> <h> <w> <latent> <hid> <layers> <chunk> <outputs: as vid, bits 0-3>
//                seq <prec> <b> <t> <gh> <gw> <cin_p> <hid_p> <layers> <all_layers> <state: bit 0 in, 1 out>
// prints per group: "<name> <calls> <FNV-1a 64 of the canonical text of those calls>"; with `dump`, the text itself on stderr
#include <dlfcn.h>
#include <link.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

struct dim3 { unsigned x, y, z; };
static uintptr_t g_base;
static std::map<uintptr_t, std::string> g_names;
static uint64_t g_hash;
static bool g_dump;
static dim3 c_grid, c_block;
static size_t c_shmem;
static void* c_stream;
static uintptr_t g_ws, g_ws_bytes;
static std::vector<void*> g_streams, g_events;      // of the current call, in order of first appearance
static uintptr_t g_next_handle = 0x500000000000ull;  // streams and events the library creates

static void put(const char* fmt, ...) {
    char buf[768];
    va_list ap;
    va_start(ap, fmt);
    const int len = vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (len >= (int)sizeof buf) { fprintf(stderr, "line too long\n"); exit(3); }
    for (int i = 0; i < len; ++i) g_hash = (g_hash ^ (unsigned char)buf[i]) * 1099511628211ull;
    if (g_dump) fputs(buf, stderr);
}
static int ordinal(std::vector<void*>& seen, void* h) {
    for (size_t i = 0; i < seen.size(); ++i) if (seen[i] == h) return (int)i;
    seen.push_back(h);
    return (int)seen.size() - 1;
}
static void put_if_ws(int word, const void* p) {
    uintptr_t v;
    memcpy(&v, p, sizeof v);
    if (v >= g_ws && v < g_ws + g_ws_bytes) put("%d:%zu ", word, (size_t)(v - g_ws));
}

// Kernels that take ONE parameter struct: the struct's name as the mangled kernel name ends with it -> sizeof.  Only these bytes
// are read: what lies behind a parameter on the launching frame may itself be a stale workspace pointer.
static const struct { const char* mangled; size_t bytes; } kStructs[] = {
    {"6Conv3P", 192}, {"7ConvC3P", 72}, {"6ConvTP", 80}, {"7ConvTP2", 96}, {"6ConvWP", 128}, {"5CellP", 56},
    {"6StoreP", 72}, {"10WideScoreP", 64}, {"5TailP", 88}, {"5Dec4P", 112}};
// Kernels with plain arguments: one letter per argument, p = a pointer (read), . = anything else (not read)
static const struct { const char* name; const char* args; } kPlain[] = {
    {"score_finalize_kernel", "p..pp.p."}, {"nhwc_to_nchw_tile_kernel", "pp..."}, {"nchw_to_nhwc_tile_kernel", "pp..."},
    {"transpose_kernel", "pp..."}, {"nchw_to_nhwc_pad_kernel", "pp...."}};

static bool ends_with(const std::string& s, const std::string& tail) {
    return s.size() >= tail.size() && s.compare(s.size() - tail.size(), tail.size(), tail) == 0;
}

extern "C" int __hipPushCallConfiguration(dim3 grid, dim3 block, size_t shmem, void* stream) {
    c_grid = grid; c_block = block; c_shmem = shmem; c_stream = stream;
    return 0;
}
extern "C" int __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* shmem, void** stream) {
    *grid = c_grid; *block = c_block; *shmem = c_shmem; *stream = c_stream;
    return 0;
}
extern "C" int hipLaunchKernel(const void* fn, dim3 grid, dim3 block, void** args, size_t shmem, void* stream) {
    const auto it = g_names.find((uintptr_t)fn - g_base);
    if (it == g_names.end()) { fprintf(stderr, "launch of an unknown kernel handle\n"); exit(3); }
    const std::string& name = it->second;
    put(" L %s %u,%u,%u %u,%u,%u %zu s%d [", name.c_str(), grid.x, grid.y, grid.z, block.x, block.y, block.z, shmem, ordinal(g_streams, stream));
    for (const auto& st : kStructs)
        if (ends_with(name, st.mangled) || ends_with(name, std::string(st.mangled) + "E")) {
            for (size_t o = 0; o + sizeof(void*) <= st.bytes; o += sizeof(void*)) put_if_ws((int)(o / sizeof(void*)), (const char*)args[0] + o);
            put("]\n");
            return 0;
        }
    for (const auto& pl : kPlain)
        if (name.find(pl.name) != std::string::npos) {
            for (int i = 0; pl.args[i]; ++i) if (pl.args[i] == 'p') put_if_ws(i, args[i]);
            put("]\n");
            return 0;
        }
    fprintf(stderr, "no parameter table entry for kernel %s\n", name.c_str());
    exit(3);
}
extern "C" int hipGetLastError(void) { return 0; }
extern "C" int hipGetDevice(int* dev) { *dev = 0; return 0; }
extern "C" int hipGetDevicePropertiesR0600(void*, int) { return 101; }          // hipErrorInvalidDevice
extern "C" int hipOccupancyMaxActiveBlocksPerMultiprocessor(int* n, const void*, int, size_t) { *n = 2; return 0; }
extern "C" int hipFuncSetAttribute(const void*, int, int) { return 0; }
extern "C" int hipEventCreateWithFlags(void** e, unsigned) { *e = (void*)(g_next_handle += 64); return 0; }
extern "C" int hipStreamCreateWithFlags(void** s, unsigned) { *s = (void*)(g_next_handle += 64); return 0; }
extern "C" int hipEventRecord(void* e, void* s) { put(" R e%d s%d\n", ordinal(g_events, e), ordinal(g_streams, s)); return 0; }
extern "C" int hipStreamWaitEvent(void* s, void* e, unsigned) { put(" W s%d e%d\n", ordinal(g_streams, s), ordinal(g_events, e)); return 0; }
extern "C" int hipMemsetAsync(void* p, int v, size_t bytes, void* s) {
    put(" M ");
    put_if_ws(0, &p);
    put("%d %zu s%d\n", v, bytes, ordinal(g_streams, s));
    return 0;
}

typedef const char* (*err_t)(void);
typedef int (*set_t)(int);
typedef size_t (*img_ws_t)(int, int, int, int, int);
typedef size_t (*vid_ws_t)(int, int, int, int, int, int, int, int);
typedef size_t (*win_ws_t)(int, int, int, int, int, int, int, int, int);
typedef size_t (*seq_ws_t)(int, int, int, int, int, int, int, int);
typedef int (*img_t)(const void*, int, int, int, long long, int, int, int, const float*, void*, size_t, int, float*, float*, float*, float*, void*);
typedef int (*vid_t)(const void*, int, int, int, long long, int, int, int, int, int, int, const float*, void*, size_t, int, float*, float*, float*,
                     float*, const float*, float*, void*);
typedef int (*win_t)(const void*, int, int, int, long long, int, int, int, int, int, int, int, const float*, void*, size_t, int, float*, float*,
                     float*, float*, void*);
typedef int (*seq_t)(const float*, int, long long, int, int, int, int, int, int, const float*, void*, size_t, float*, int, const float*, float*, void*);

// made-up addresses, 1 TiB apart: x, the weight blob, the workspace, six outputs / states, the caller's stream.  Their low halves
// are no small integer: an int field next to padding that holds the stale upper half of a pointer is then no workspace address.
static void* fake(int i) { return (void*)(0x100080000000ull + 0x10000000000ull * (uintptr_t)i); }
static float* out(long mask, int bit) { return (mask >> bit & 1) ? (float*)fake(3 + bit) : nullptr; }

int main(int argc, char** argv) {
    if (argc != 4 && argc != 5) return 2;
    g_dump = argc == 5;
    void* h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
    if (!h) { fprintf(stderr, "%s\n", dlerror()); return 1; }
    struct link_map* lm = nullptr;
    dlinfo(h, RTLD_DI_LINKMAP, &lm);
    g_base = lm->l_addr;
    FILE* syms = fopen(argv[2], "r");
    if (!syms) return 1;
    unsigned long off;
    for (char name[400]; fscanf(syms, "%lx %399s", &off, name) == 2;) g_names.emplace(off, name);
    fclose(syms);
    const err_t last_error = (err_t)dlsym(h, "vad_last_error");
    const img_ws_t img_ws = (img_ws_t)dlsym(h, "vad_img_workspace_bytes_c");
    const vid_ws_t vid_ws = (vid_ws_t)dlsym(h, "vad_vid_workspace_bytes_c");
    const win_ws_t win_ws = (win_ws_t)dlsym(h, "vad_vid_windows_workspace_bytes_c");
    const seq_ws_t seq_ws = (seq_ws_t)dlsym(h, "vad_convlstm_seq_workspace_bytes");
    const img_t img = (img_t)dlsym(h, "vad_img_score_c");
    const vid_t vid = (vid_t)dlsym(h, "vad_vid_score_s");
    const win_t win = (win_t)dlsym(h, "vad_vid_score_windows_c");
    const seq_t seq = (seq_t)dlsym(h, "vad_convlstm_seq");
    if (!last_error || !img_ws || !vid_ws || !win_ws || !seq_ws || !img || !vid || !win || !seq) return 1;
    FILE* script = fopen(argv[3], "r");
    if (!script) return 1;
    g_ws = (uintptr_t)fake(2);
    void* const ws = fake(2);
    const float* const packed = (const float*)fake(1);
    void* const stream = fake(9);
    std::string group;
    long calls = 0;
    auto flush = [&] {
        if (!group.empty()) printf("%s %ld %016llx\n", group.c_str(), calls, (unsigned long long)g_hash);
    };
    char line[512], word[64], sym[128];
    while (fgets(line, sizeof line, script)) {
        long a[16] = {};
        const int n = sscanf(line, "%63s %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld", word, a, a + 1, a + 2, a + 3, a + 4, a + 5, a + 6, a + 7,
                             a + 8, a + 9, a + 10, a + 11, a + 12, a + 13) - 1;
        const std::string w = n >= 0 ? word : "";
        if (w == "group" && sscanf(line, "%*s %127s", sym) == 1) {
            flush();
            group = sym; calls = 0; g_hash = 14695981039346656037ull;
            continue;
        }
        if (w == "set" && sscanf(line, "%*s %127s %ld", sym, a) == 2) {
            const set_t set = strncmp(sym, "vad_debug_set_", 14) ? nullptr : (set_t)dlsym(h, sym);
            if (!set) { fprintf(stderr, "no switch %s\n", sym); return 1; }
            set((int)a[0]);
            continue;
        }
        put("%s", line);
        g_streams.clear(); g_events.clear();
        int rc;
        if (w == "img" && n == 9) {
            g_ws_bytes = img_ws((int)a[7], (int)a[4], (int)a[5], (int)a[6], (int)a[2]);
            rc = img(fake(0), (int)a[0], (int)a[1], (int)a[2], a[3], (int)a[4], (int)a[5], (int)a[6], packed, ws, g_ws_bytes, (int)a[7], out(a[8], 0),
                     out(a[8], 1), out(a[8], 2), out(a[8], 3), stream);
        } else if (w == "vid" && n == 12) {
            g_ws_bytes = vid_ws((int)a[10], (int)a[4], (int)a[5], (int)a[6], (int)a[7], (int)a[8], (int)a[9], (int)a[2]);
            rc = vid(fake(0), (int)a[0], (int)a[1], (int)a[2], a[3], (int)a[4], (int)a[5], (int)a[6], (int)a[7], (int)a[8], (int)a[9], packed, ws, g_ws_bytes,
                     (int)a[10], out(a[11], 0), out(a[11], 1), out(a[11], 2), out(a[11], 3), out(a[11], 4), out(a[11], 5), stream);
        } else if (w == "win" && n == 13) {
            g_ws_bytes = win_ws((int)a[11], (int)a[4], (int)a[5], (int)a[6], (int)a[7], (int)a[8], (int)a[9], (int)a[10], (int)a[2]);
            rc = win(fake(0), (int)a[0], (int)a[1], (int)a[2], a[3], (int)a[4], (int)a[5], (int)a[6], (int)a[7], (int)a[8], (int)a[9], (int)a[10], packed, ws,
                     g_ws_bytes, (int)a[11], out(a[12], 0), out(a[12], 1), out(a[12], 2), out(a[12], 3), stream);
        } else if (w == "seq" && n == 10) {
            g_ws_bytes = seq_ws((int)a[1], (int)a[2], (int)a[3], (int)a[4], (int)a[5], (int)a[6], (int)a[7], (int)a[8]);
            rc = seq((const float*)fake(0), (int)a[0], a[1], (int)a[2], (int)a[3], (int)a[4], (int)a[5], (int)a[6], (int)a[7], packed, ws, g_ws_bytes,
                     (float*)fake(3), (int)a[8], out(a[9], 0) ? (const float*)fake(7) : nullptr, out(a[9], 1) ? (float*)fake(8) : nullptr, stream);
        } else {
            fprintf(stderr, "bad script line: %s", line);
            return 1;
        }
        put(" ws %zu rc %d %s\n", (size_t)g_ws_bytes, rc, rc ? last_error() : "");
        ++calls;
    }
    flush();
    fclose(script);
    return 0;
}
