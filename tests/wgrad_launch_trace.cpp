// Stand-alone host program for tests/test_wgrad_plan.py: loads libvad_hip.so and digests what vad_conv_wgrad WOULD launch for a
// grid of arguments under each of the 32 debug-switch settings - kernel symbol, grid, block, dynamic LDS, the integer fields of
// the kernel's parameter struct, and the reduce launch that follows - by defining the three HIP launch entry points itself.
// Nothing reaches a GPU, none is needed.
// usage: wgrad_launch_trace <libvad_hip.so> <symbols: "hex-offset name" per line> <cin,..> <ncols,..> <n,..> <h,..> <w,..>
// prints one line per switch setting: "<pairs><split><ring_f32> <calls> <FNV-1a 64 of the canonical text of those calls>"
#include <dlfcn.h>
#include <link.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

struct dim3 { unsigned x, y, z; };
static uintptr_t g_base;
static std::map<uintptr_t, std::string> g_names;
static uint64_t g_hash;
static dim3 c_grid, c_block;
static size_t c_shmem;
static void* c_stream;
static int g_nlaunch;

static void put(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    const int len = vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    for (int i = 0; i < len && i < (int)sizeof buf; ++i) g_hash = (g_hash ^ (unsigned char)buf[i]) * 1099511628211ull;
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
    put(" L %s %u,%u,%u %u,%u,%u %zu [", name.c_str(), grid.x, grid.y, grid.z, block.x, block.y, block.z, shmem);
    if (g_nlaunch++ == 0) {          // the gradient kernel: one struct of three pointers, then ints (WgradP 10; WgradRingP 9, then padding)
        const int* q = (const int*)((const char*)args[0] + 3 * sizeof(void*));
        const int nints = name.find("conv_wgrad_ring_kernel") != std::string::npos ? 9 : 10;
        for (int i = 0; i < nints; ++i) put("%d ", q[i]);
    } else {                         // wgrad_reduce_kernel(ws, splits, taps, cin, ncols, layout, dst)
        for (int i = 1; i <= 5; ++i) put("%d ", *(const int*)args[i]);
    }
    put("]");
    return 0;
}
extern "C" int hipGetLastError(void) { return 0; }

typedef int (*wgrad_t)(const float*, const float*, float*, float*, int, int, int, int, int, int, int, int, void*);
typedef int (*set_t)(int);

static std::vector<int> ints(const char* s) {
    std::vector<int> v;
    for (char* e; *s; s = *e ? e + 1 : e) v.push_back((int)strtol(s, &e, 10));
    return v;
}

int main(int argc, char** argv) {
    if (argc != 8) return 2;
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
    wgrad_t wgrad = (wgrad_t)dlsym(h, "vad_conv_wgrad");
    set_t pairs = (set_t)dlsym(h, "vad_debug_set_wgrad_pairs"), split = (set_t)dlsym(h, "vad_debug_set_wgrad_split"),
          ring = (set_t)dlsym(h, "vad_debug_set_wgrad_ring_f32");
    if (!wgrad || !pairs || !split || !ring) return 1;
    const std::vector<int> cins = ints(argv[3]), ncs = ints(argv[4]), ns = ints(argv[5]), hs = ints(argv[6]), ws = ints(argv[7]);
    static float dummy[4];           // never dereferenced: nothing is launched
    for (int a = 0; a < 4; ++a) for (int b = 0; b < 4; ++b) for (int c = 0; c < 2; ++c) {
        pairs(a); split(b); ring(c);
        g_hash = 14695981039346656037ull;
        long calls = 0;
        for (int prec = 0; prec < 4; ++prec) for (int taps : {1, 9}) for (int cin : cins) for (int nc : ncs) for (int n : ns) for (int hh : hs)
            for (int w : ws) {
                put("%d %d %d %d %d %d %d:", prec, taps, cin, nc, n, hh, w);
                g_nlaunch = 0;
                const int rc = wgrad(dummy, dummy, dummy, dummy, n, hh, w, cin, nc, taps, taps == 9 ? 0 : 4, prec, nullptr);
                put(" rc %d launches %d\n", rc, g_nlaunch);
                ++calls;
            }
        printf("%d%d%d %ld %016llx\n", a, b, c, calls, (unsigned long long)g_hash);
    }
    return 0;
}
