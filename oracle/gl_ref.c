/* oracle/gl_ref.c — TEST INFRASTRUCTURE.  A headless OpenGL ES 3 harness that runs the reference's OWN, unmodified shader
 * strings (what SplatMaterial3D.build() returns, dumped by oracle/shader_dump.mjs) with the reference's blend state on Mesa's
 * software rasteriser (llvmpipe, swrast_dri.so), loaded through the DRI interface without X, EGL or OSMesa.  Loaded with ctypes
 * by oracle/make_golden_gl.py, which records what it computes into tests/golden/gl_{vertex,frames}_ref.npz; nothing of this
 * runs in the test suite or is needed where the GPU tests run.
 *
 * What GL executes here as the reference's WebGL2 draw does: the vertex and fragment shaders, the data-texture reads through
 * texture() with NEAREST filtering at the reference's texture sizes (4096 x 1024 * 2^k, SplatMesh.js:643-647), the instanced
 * quad (SplatGeometry.js:11-37), rasterisation and clipping, the depth test of `depthTest: true, depthWrite: false` and
 * NormalBlending into an RGBA8 target (SplatMaterial3D.js:65-75).
 * The two stand-ins left: the three.js r160 WebGLProgram prefix (three_prefix() below) and the texel packing (oracle/texel_pack.h,
 * shared with oracle/shader_harness.cpp).
 *
 * Exports:
 *   glref_init(version, renderer, cap)                             creates the context; GL_VERSION / GL_RENDERER strings
 *   glref_capture_vertices(vert, frag, scene, uniforms, splat_index, count, out)   transform feedback of gl_Position, vColor, vPosition
 *   glref_draw_frame(vert, frag, scene, uniforms, order, count, w, h, dst_depth, depth_format, dst_rgba, out_rgba8)
 *   glref_run_fragment(frag, count, v_position, v_color, out_rgba, out_discard)   the fragment shader at given varyings
 * All return 0 on success, or a negative code after printing the GL error / info log to stderr.
 *
 * No GLES3/ headers are assumed: enums come from GL/glext.h (the same values) and the entry points are declared locally as
 * function-pointer types. */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <GL/gl.h>
#include <GL/glext.h>
#include <GL/internal/dri_interface.h>

#include "texel_pack.h"

/* ---------------------------------------------------------------------------------------------------- the scene / uniforms
 * The same structs oracle/make_golden_raster.py passes to oracle/shader_harness.cpp. */
typedef struct {
    uint32_t count, sh_degree_stored, cov_half, sh_u8;
    const float* centers;
    const uint8_t* rgba;
    const float* cov;
    const uint16_t* cov16;
    const float* sh;              /* what the sampler returns: fp16 values widened, or byte / 255 (sh_u8) */
    const uint32_t* scene_idx;    /* [n] or NULL */
} HarnessScene;

typedef struct {
    float model_view[16], projection[16], view_matrix[16], camera_position[3];
    float focal[2], viewport[2], ortho_zoom, inverse_focal_adjustment, splat_scale;
    int32_t orthographic, point_cloud, sh_degree, sh_8bit, fade_in_complete, scene_count;
    float scene_center[3], fade_start_radius;
    float transforms[32][16], scene_opacity[32], sh8_min[32], sh8_max[32];
    int32_t scene_visibility[32];
} HarnessUniforms;

/* ---------------------------------------------------------------------------------------------------- GL entry points */
#define GL_FUNCS(X) \
    X(const GLubyte*, GetString, (GLenum)) \
    X(GLenum, GetError, (void)) \
    X(GLuint, CreateShader, (GLenum)) \
    X(void, ShaderSource, (GLuint, GLsizei, const GLchar* const*, const GLint*)) \
    X(void, CompileShader, (GLuint)) \
    X(void, GetShaderiv, (GLuint, GLenum, GLint*)) \
    X(void, GetShaderInfoLog, (GLuint, GLsizei, GLsizei*, GLchar*)) \
    X(GLuint, CreateProgram, (void)) \
    X(void, AttachShader, (GLuint, GLuint)) \
    X(void, LinkProgram, (GLuint)) \
    X(void, GetProgramiv, (GLuint, GLenum, GLint*)) \
    X(void, GetProgramInfoLog, (GLuint, GLsizei, GLsizei*, GLchar*)) \
    X(void, UseProgram, (GLuint)) \
    X(void, DeleteProgram, (GLuint)) \
    X(void, DeleteShader, (GLuint)) \
    X(void, TransformFeedbackVaryings, (GLuint, GLsizei, const GLchar* const*, GLenum)) \
    X(GLint, GetUniformLocation, (GLuint, const GLchar*)) \
    X(GLint, GetAttribLocation, (GLuint, const GLchar*)) \
    X(void, Uniform1i, (GLint, GLint)) \
    X(void, Uniform1f, (GLint, GLfloat)) \
    X(void, Uniform2f, (GLint, GLfloat, GLfloat)) \
    X(void, Uniform3f, (GLint, GLfloat, GLfloat, GLfloat)) \
    X(void, Uniform1fv, (GLint, GLsizei, const GLfloat*)) \
    X(void, Uniform1iv, (GLint, GLsizei, const GLint*)) \
    X(void, UniformMatrix4fv, (GLint, GLsizei, GLboolean, const GLfloat*)) \
    X(void, GenBuffers, (GLsizei, GLuint*)) \
    X(void, DeleteBuffers, (GLsizei, const GLuint*)) \
    X(void, BindBuffer, (GLenum, GLuint)) \
    X(void, BufferData, (GLenum, GLsizeiptr, const void*, GLenum)) \
    X(void, BindBufferBase, (GLenum, GLuint, GLuint)) \
    X(void*, MapBufferRange, (GLenum, GLintptr, GLsizeiptr, GLbitfield)) \
    X(GLboolean, UnmapBuffer, (GLenum)) \
    X(void, GenVertexArrays, (GLsizei, GLuint*)) \
    X(void, DeleteVertexArrays, (GLsizei, const GLuint*)) \
    X(void, BindVertexArray, (GLuint)) \
    X(void, EnableVertexAttribArray, (GLuint)) \
    X(void, VertexAttribPointer, (GLuint, GLint, GLenum, GLboolean, GLsizei, const void*)) \
    X(void, VertexAttribIPointer, (GLuint, GLint, GLenum, GLsizei, const void*)) \
    X(void, VertexAttribDivisor, (GLuint, GLuint)) \
    X(void, GenTextures, (GLsizei, GLuint*)) \
    X(void, DeleteTextures, (GLsizei, const GLuint*)) \
    X(void, BindTexture, (GLenum, GLuint)) \
    X(void, ActiveTexture, (GLenum)) \
    X(void, TexImage2D, (GLenum, GLint, GLint, GLsizei, GLsizei, GLint, GLenum, GLenum, const void*)) \
    X(void, TexParameteri, (GLenum, GLenum, GLint)) \
    X(void, PixelStorei, (GLenum, GLint)) \
    X(void, GenFramebuffers, (GLsizei, GLuint*)) \
    X(void, DeleteFramebuffers, (GLsizei, const GLuint*)) \
    X(void, BindFramebuffer, (GLenum, GLuint)) \
    X(void, GenRenderbuffers, (GLsizei, GLuint*)) \
    X(void, DeleteRenderbuffers, (GLsizei, const GLuint*)) \
    X(void, BindRenderbuffer, (GLenum, GLuint)) \
    X(void, RenderbufferStorage, (GLenum, GLenum, GLsizei, GLsizei)) \
    X(void, FramebufferRenderbuffer, (GLenum, GLenum, GLenum, GLuint)) \
    X(GLenum, CheckFramebufferStatus, (GLenum)) \
    X(void, Viewport, (GLint, GLint, GLsizei, GLsizei)) \
    X(void, ClearColor, (GLfloat, GLfloat, GLfloat, GLfloat)) \
    X(void, ClearDepthf, (GLfloat)) \
    X(void, Clear, (GLbitfield)) \
    X(void, Enable, (GLenum)) \
    X(void, Disable, (GLenum)) \
    X(void, DepthFunc, (GLenum)) \
    X(void, DepthMask, (GLboolean)) \
    X(void, ColorMask, (GLboolean, GLboolean, GLboolean, GLboolean)) \
    X(void, BlendEquation, (GLenum)) \
    X(void, BlendFuncSeparate, (GLenum, GLenum, GLenum, GLenum)) \
    X(void, BeginTransformFeedback, (GLenum)) \
    X(void, EndTransformFeedback, (void)) \
    X(void, DrawArraysInstanced, (GLenum, GLint, GLsizei, GLsizei)) \
    X(void, DrawArrays, (GLenum, GLint, GLsizei)) \
    X(void, DrawElementsInstanced, (GLenum, GLsizei, GLenum, const void*, GLsizei)) \
    X(void, ReadPixels, (GLint, GLint, GLsizei, GLsizei, GLenum, GLenum, void*)) \
    X(void, Finish, (void))

#define DECL(ret, name, args) typedef ret(*PFN_##name) args; static PFN_##name gl_##name;
GL_FUNCS(DECL)
#undef DECL
#define GL(name) gl_##name          /* <GL/gl.h> declares the GL 1.x prototypes: ours live under their own names */

/* ---------------------------------------------------------------------------------------------------- the DRI context */
static const __DRIcoreExtension* g_core;
static const __DRIswrastExtension* g_swrast;
static __DRIscreen* g_screen;
static __DRIdrawable* g_drawable;
static __DRIcontext* g_context;

/* The drawable is a dummy: every draw goes into an FBO. */
static void get_drawable_info(__DRIdrawable* d, int* x, int* y, int* w, int* h, void* p) {
    (void)d; (void)p;
    *x = 0; *y = 0; *w = 1; *h = 1;
}
static void put_image(__DRIdrawable* d, int op, int x, int y, int w, int h, char* data, void* p) {
    (void)d; (void)op; (void)x; (void)y; (void)w; (void)h; (void)data; (void)p;
}
static void get_image(__DRIdrawable* d, int x, int y, int w, int h, char* data, void* p) {
    (void)d; (void)x; (void)y; (void)p;
    memset(data, 0, (size_t)w * (size_t)h * 4);
}
static const __DRIswrastLoaderExtension g_loader = {
    .base = {__DRI_SWRAST_LOADER, 1}, .getDrawableInfo = get_drawable_info, .putImage = put_image, .getImage = get_image};
static const __DRIextension* g_loader_exts[] = {&g_loader.base, NULL};

static int gl_check(const char* where) {
    GLenum e = GL(GetError)();
    if (e != GL_NO_ERROR) { fprintf(stderr, "gl_ref: GL error 0x%04x at %s\n", e, where); return -1; }
    return 0;
}

int glref_init(char* version, char* renderer, int cap) {
    if (g_context) goto strings;
    /* llvmpipe's thread count is fixed (its rasteriser bins by tile: results do not depend on it, the run's timing does) */
    setenv("LP_NUM_THREADS", "4", 1);
    void* glapi = dlopen("libglapi.so.0", RTLD_NOW | RTLD_GLOBAL);
    if (!glapi) { fprintf(stderr, "gl_ref: %s\n", dlerror()); return -1; }
    const char* dri_path = getenv("GLREF_DRI");
    void* dri = dlopen(dri_path ? dri_path : "/usr/lib/x86_64-linux-gnu/dri/swrast_dri.so", RTLD_NOW | RTLD_GLOBAL);
    if (!dri) { fprintf(stderr, "gl_ref: %s\n", dlerror()); return -2; }
    typedef const __DRIextension** (*GetExt)(void);
    GetExt get = (GetExt)dlsym(dri, "__driDriverGetExtensions_swrast");
    if (!get) { fprintf(stderr, "gl_ref: no __driDriverGetExtensions_swrast\n"); return -3; }
    const __DRIextension** ext = get();
    for (int i = 0; ext[i]; i++) {
        if (!strcmp(ext[i]->name, __DRI_CORE)) g_core = (const __DRIcoreExtension*)ext[i];
        if (!strcmp(ext[i]->name, __DRI_SWRAST)) g_swrast = (const __DRIswrastExtension*)ext[i];
    }
    if (!g_core || !g_swrast || g_swrast->base.version < 4) { fprintf(stderr, "gl_ref: DRI_Core / DRI_SWRast v4 missing\n"); return -4; }
    const __DRIconfig** configs = NULL;
    g_screen = g_swrast->createNewScreen2(0, g_loader_exts, ext, &configs, NULL);
    if (!g_screen || !configs || !configs[0]) { fprintf(stderr, "gl_ref: createNewScreen2 failed\n"); return -5; }
    const __DRIconfig* cfg = configs[0];
    for (int i = 0; configs[i]; i++) {                       /* an RGBA8 config without MSAA (the FBO decides what is drawn) */
        unsigned r = 0, a = 0, s = 0;
        g_core->getConfigAttrib(configs[i], __DRI_ATTRIB_RED_SIZE, &r);
        g_core->getConfigAttrib(configs[i], __DRI_ATTRIB_ALPHA_SIZE, &a);
        g_core->getConfigAttrib(configs[i], __DRI_ATTRIB_SAMPLES, &s);
        if (r == 8 && a == 8 && s == 0) { cfg = configs[i]; break; }
    }
    g_drawable = g_swrast->createNewDrawable(g_screen, cfg, NULL);
    const uint32_t attribs[] = {__DRI_CTX_ATTRIB_MAJOR_VERSION, 3, __DRI_CTX_ATTRIB_MINOR_VERSION, 0};
    unsigned err = 0;
    g_context = g_swrast->createContextAttribs(g_screen, __DRI_API_GLES3, cfg, NULL, 2, attribs, &err, NULL);
    if (!g_context) { fprintf(stderr, "gl_ref: createContextAttribs(GLES3) failed: %u\n", err); return -6; }
    if (!g_core->bindContext(g_context, g_drawable, g_drawable)) { fprintf(stderr, "gl_ref: bindContext failed\n"); return -7; }
    typedef void* (*GetProc)(const char*);
    GetProc gp = (GetProc)dlsym(glapi, "_glapi_get_proc_address");
    if (!gp) { fprintf(stderr, "gl_ref: no _glapi_get_proc_address\n"); return -8; }
#define LOAD(ret, name, args) \
    gl_##name = (PFN_##name)gp("gl" #name); \
    if (!gl_##name) { fprintf(stderr, "gl_ref: no gl" #name "\n"); return -9; }
    GL_FUNCS(LOAD)
#undef LOAD
strings:
    snprintf(version, cap, "%s", (const char*)GL(GetString)(GL_VERSION));
    snprintf(renderer, cap, "%s", (const char*)GL(GetString)(GL_RENDERER));
    return 0;
}

/* ---------------------------------------------------------------------------------------------------- programs
 * three.js r160 WebGLProgram (src/renderers/webgl/WebGLProgram.js) for a ShaderMaterial on a WebGL2 context: the version line and
 * the GLSL1 -> 3 defines (`attribute` / `varying` / `texture2D`, and for the fragment stage `pc_fragColor` standing in for
 * gl_FragColor), the precision block of generatePrecision() for precision 'highp', the SHADER_TYPE / SHADER_NAME defines, and the
 * built-in uniforms and the `position` attribute that the splat shaders read.  `#include <common>` resolves to the common chunk;
 * the splat shaders use nothing of it, so it stays empty here.  This prefix is a stand-in (with the texel packing, the only one). */
static char* three_prefix(const char* body, int fragment) {
    static const char* precision =
        "precision highp float;\nprecision highp int;\nprecision highp sampler2D;\nprecision highp samplerCube;\n"
        "precision highp sampler3D;\nprecision highp sampler2DArray;\nprecision highp sampler2DShadow;\n"
        "precision highp samplerCubeShadow;\nprecision highp sampler2DArrayShadow;\nprecision highp isampler2D;\n"
        "precision highp isampler3D;\nprecision highp isamplerCube;\nprecision highp isampler2DArray;\n"
        "precision highp usampler2D;\nprecision highp usampler3D;\nprecision highp usamplerCube;\n"
        "precision highp usampler2DArray;\n#define HIGH_PRECISION\n";
    static const char* vert =
        "#version 300 es\n#define attribute in\n#define varying out\n#define texture2D texture\n%s"
        "#define SHADER_TYPE ShaderMaterial\n#define SHADER_NAME ShaderMaterial\n"
        "uniform mat4 modelMatrix;\nuniform mat4 modelViewMatrix;\nuniform mat4 projectionMatrix;\nuniform mat4 viewMatrix;\n"
        "uniform mat3 normalMatrix;\nuniform vec3 cameraPosition;\nuniform bool isOrthographic;\n"
        "attribute vec3 position;\n";
    static const char* frag =
        "#version 300 es\n#define varying in\nlayout(location = 0) out highp vec4 pc_fragColor;\n#define gl_FragColor pc_fragColor\n"
        "#define gl_FragDepthEXT gl_FragDepth\n#define texture2D texture\n%s"
        "#define SHADER_TYPE ShaderMaterial\n#define SHADER_NAME ShaderMaterial\n"
        "uniform mat4 viewMatrix;\nuniform vec3 cameraPosition;\nuniform bool isOrthographic;\n";
    char head[4096];
    snprintf(head, sizeof head, fragment ? frag : vert, precision);
    const char* inc = "#include <common>";
    size_t n = strlen(head) + strlen(body) + 1;
    char* out = (char*)malloc(n);
    strcpy(out, head);
    const char* p = strstr(body, inc);
    if (p) {
        strncat(out, body, (size_t)(p - body));
        strcat(out, body + (p - body) + strlen(inc));
    } else {
        strcat(out, body);
    }
    return out;
}

static GLuint compile(GLenum type, const char* src) {
    GLuint s = GL(CreateShader)(type);
    GL(ShaderSource)(s, 1, &src, NULL);
    GL(CompileShader)(s);
    GLint ok = 0;
    GL(GetShaderiv)(s, GL_COMPILE_STATUS, &ok);
    if (!ok) {
        char log[4096];
        GL(GetShaderInfoLog)(s, sizeof log, NULL, log);
        fprintf(stderr, "gl_ref: %s shader: %s\n", type == GL_VERTEX_SHADER ? "vertex" : "fragment", log);
        GL(DeleteShader)(s);
        return 0;
    }
    return s;
}

/* raw = 1: vert / frag are complete GLSL ES 3.00 (our own helper programs); 0: the reference's strings behind three's prefix */
static GLuint program(const char* vert, const char* frag, int raw, int feedback) {
    char* v = raw ? NULL : three_prefix(vert, 0);
    char* f = raw ? NULL : three_prefix(frag, 1);
    GLuint vs = compile(GL_VERTEX_SHADER, raw ? vert : v), fs = compile(GL_FRAGMENT_SHADER, raw ? frag : f);
    free(v); free(f);
    if (!vs || !fs) return 0;
    GLuint p = GL(CreateProgram)();
    GL(AttachShader)(p, vs);
    GL(AttachShader)(p, fs);
    if (feedback) {
        const char* names[] = {"gl_Position", "vColor", "vPosition"};
        GL(TransformFeedbackVaryings)(p, 3, names, GL_INTERLEAVED_ATTRIBS);
    }
    GL(LinkProgram)(p);
    GL(DeleteShader)(vs);
    GL(DeleteShader)(fs);
    GLint ok = 0;
    GL(GetProgramiv)(p, GL_LINK_STATUS, &ok);
    if (!ok) {
        char log[4096];
        GL(GetProgramInfoLog)(p, sizeof log, NULL, log);
        fprintf(stderr, "gl_ref: link: %s\n", log);
        GL(DeleteProgram)(p);
        return 0;
    }
    return p;
}

/* ---------------------------------------------------------------------------------------------------- data textures */
typedef struct { GLuint tex[6]; int ntex; } Textures;

/* SplatMesh.js:643-647: 4096 x 1024, the height doubled until the texels hold every splat's elements */
static void ref_size(uint64_t elements_per_texel, uint64_t elements_per_splat, uint64_t n, int* w, int* h) {
    uint64_t W = 4096, H = 1024;
    while (W * H * elements_per_texel < n * elements_per_splat) H *= 2;
    *w = (int)W; *h = (int)H;
}

static GLuint upload(GLenum unit, GLint internal, int w, int h, GLenum format, GLenum type, const void* data) {
    GLuint t;
    GL(GenTextures)(1, &t);
    GL(ActiveTexture)(GL_TEXTURE0 + unit);
    GL(BindTexture)(GL_TEXTURE_2D, t);
    GL(PixelStorei)(GL_UNPACK_ALIGNMENT, 1);
    GL(TexImage2D)(GL_TEXTURE_2D, 0, internal, w, h, 0, format, type, data);
    /* three.js DataTexture defaults: NEAREST / NEAREST, no mipmaps, CLAMP_TO_EDGE */
    GL(TexParameteri)(GL_TEXTURE_2D, GL_TEXTURE_MIN_FILTER, GL_NEAREST);
    GL(TexParameteri)(GL_TEXTURE_2D, GL_TEXTURE_MAG_FILTER, GL_NEAREST);
    GL(TexParameteri)(GL_TEXTURE_2D, GL_TEXTURE_WRAP_S, GL_CLAMP_TO_EDGE);
    GL(TexParameteri)(GL_TEXTURE_2D, GL_TEXTURE_WRAP_T, GL_CLAMP_TO_EDGE);
    return t;
}

static void set_sampler(GLuint prog, const char* name, int unit) {
    GLint l = GL(GetUniformLocation)(prog, name);
    if (l >= 0) GL(Uniform1i)(l, unit);
}
static void set_size(GLuint prog, const char* name, int w, int h) {
    GLint l = GL(GetUniformLocation)(prog, name);
    if (l >= 0) GL(Uniform2f)(l, (float)w, (float)h);
}

/* Textures as SplatMesh.setupDataTextures makes them (formats :691-741 / :797-886); units: 0 centersColors, 1 covariances,
 * 2 covariancesHalfFloat, 3 sphericalHarmonics, 4 sceneIndexes, 5 (R/G/B multi-texture SH: never selected, a 2x2 dummy) */
static int data_textures(GLuint prog, const HarnessScene* sc, Textures* t) {
    const uint32_t n = sc->count;
    int w, h;
    t->ntex = 0;
    ref_size(4, 4, n, &w, &h);
    uint32_t* cc = (uint32_t*)malloc(sizeof(uint32_t) * 4 * tp_texels(w, h));
    tp_pack_centers_colors(n, sc->centers, sc->rgba, w, h, cc);
    t->tex[t->ntex++] = upload(0, GL_RGBA32UI, w, h, GL_RGBA_INTEGER, GL_UNSIGNED_INT, cc);
    free(cc);
    set_sampler(prog, "centersColorsTexture", 0);
    set_size(prog, "centersColorsTextureSize", w, h);
    static const uint32_t zero[16] = {0};
    if (sc->cov_half) {
        ref_size(6, 6, n, &w, &h);
        uint32_t* ch = (uint32_t*)malloc(sizeof(uint32_t) * 4 * tp_texels(w, h));
        tp_pack_covariances_half(n, sc->cov16, w, h, ch);
        t->tex[t->ntex++] = upload(2, GL_RGBA32UI, w, h, GL_RGBA_INTEGER, GL_UNSIGNED_INT, ch);
        free(ch);
        t->tex[t->ntex++] = upload(1, GL_RGBA32F, 2, 2, GL_RGBA, GL_FLOAT, zero);
    } else {
        ref_size(4, 6, n, &w, &h);
        float* cf = (float*)malloc(sizeof(float) * 4 * tp_texels(w, h));
        tp_pack_covariances(n, sc->cov, w, h, cf);
        t->tex[t->ntex++] = upload(1, GL_RGBA32F, w, h, GL_RGBA, GL_FLOAT, cf);
        free(cf);
        t->tex[t->ntex++] = upload(2, GL_RGBA32UI, 2, 2, GL_RGBA_INTEGER, GL_UNSIGNED_INT, zero);   /* SplatMesh.js:744-748 */
    }
    set_sampler(prog, "covariancesTexture", 1);
    set_sampler(prog, "covariancesTextureHalfFloat", 2);
    set_size(prog, "covariancesTextureSize", w, h);
    GLint l = GL(GetUniformLocation)(prog, "covariancesAreHalfFloat");
    if (l >= 0) GL(Uniform1i)(l, sc->cov_half ? 1 : 0);
    const uint32_t ncoef = sc->sh_degree_stored == 0 ? 0 : (sc->sh_degree_stored == 1 ? 9 : 24);
    if (ncoef) {
        ref_size(4, tp_sh_stride(ncoef), n, &w, &h);
        float* sf = (float*)malloc(sizeof(float) * 4 * tp_texels(w, h));
        tp_pack_sh(n, ncoef, sc->sh, w, h, sf);
        if (sc->sh_u8) {                                     /* compression level 2: UnsignedByteType RGBA -> RGBA8 (:805) */
            uint8_t* b = (uint8_t*)malloc(4 * tp_texels(w, h));
            for (size_t i = 0; i < 4 * tp_texels(w, h); i++) b[i] = (uint8_t)lrintf(sf[i] * 255.0f);   /* exact: sh = byte / 255 */
            t->tex[t->ntex++] = upload(3, GL_RGBA8, w, h, GL_RGBA, GL_UNSIGNED_BYTE, b);
            free(b);
        } else {                                             /* HalfFloatType RGBA -> RGBA16F; the values are fp16 already */
            t->tex[t->ntex++] = upload(3, GL_RGBA16F, w, h, GL_RGBA, GL_FLOAT, sf);
        }
        free(sf);
        set_size(prog, "sphericalHarmonicsTextureSize", w, h);
    } else {
        t->tex[t->ntex++] = upload(3, GL_RGBA16F, 2, 2, GL_RGBA, GL_FLOAT, zero);
    }
    set_sampler(prog, "sphericalHarmonicsTexture", 3);
    t->tex[t->ntex++] = upload(5, GL_RGBA16F, 2, 2, GL_RGBA, GL_FLOAT, zero);
    set_sampler(prog, "sphericalHarmonicsTextureR", 5);
    set_sampler(prog, "sphericalHarmonicsTextureG", 5);
    set_sampler(prog, "sphericalHarmonicsTextureB", 5);
    ref_size(1, 4, n, &w, &h);
    uint32_t* si = (uint32_t*)malloc(sizeof(uint32_t) * tp_texels(w, h));
    if (sc->scene_idx) tp_pack_scene_indexes(n, sc->scene_idx, w, h, si);
    else memset(si, 0, sizeof(uint32_t) * tp_texels(w, h));
    t->tex[t->ntex++] = upload(4, GL_R32UI, w, h, GL_RED_INTEGER, GL_UNSIGNED_INT, si);
    free(si);
    set_sampler(prog, "sceneIndexesTexture", 4);
    set_size(prog, "sceneIndexesTextureSize", w, h);
    return gl_check("data textures");
}

static void uniforms(GLuint prog, const HarnessUniforms* u) {
#define LOC(name) GL(GetUniformLocation)(prog, name)
    GLint l;
    if ((l = LOC("modelViewMatrix")) >= 0) GL(UniformMatrix4fv)(l, 1, GL_FALSE, u->model_view);
    if ((l = LOC("projectionMatrix")) >= 0) GL(UniformMatrix4fv)(l, 1, GL_FALSE, u->projection);
    if ((l = LOC("viewMatrix")) >= 0) GL(UniformMatrix4fv)(l, 1, GL_FALSE, u->view_matrix);
    if ((l = LOC("cameraPosition")) >= 0) GL(Uniform3f)(l, u->camera_position[0], u->camera_position[1], u->camera_position[2]);
    if ((l = LOC("focal")) >= 0) GL(Uniform2f)(l, u->focal[0], u->focal[1]);
    if ((l = LOC("viewport")) >= 0) GL(Uniform2f)(l, u->viewport[0], u->viewport[1]);
    /* SplatMesh.updateUniforms: basisViewport = 1 / viewport, in fp64 then stored as fp32 (the shim: 1.0f / v) */
    if ((l = LOC("basisViewport")) >= 0) GL(Uniform2f)(l, 1.0f / u->viewport[0], 1.0f / u->viewport[1]);
    if ((l = LOC("orthoZoom")) >= 0) GL(Uniform1f)(l, u->ortho_zoom);
    if ((l = LOC("orthographicMode")) >= 0) GL(Uniform1i)(l, u->orthographic);
    if ((l = LOC("pointCloudModeEnabled")) >= 0) GL(Uniform1i)(l, u->point_cloud);
    if ((l = LOC("inverseFocalAdjustment")) >= 0) GL(Uniform1f)(l, u->inverse_focal_adjustment);
    if ((l = LOC("splatScale")) >= 0) GL(Uniform1f)(l, u->splat_scale);
    if ((l = LOC("sphericalHarmonicsDegree")) >= 0) GL(Uniform1i)(l, u->sh_degree);
    if ((l = LOC("sphericalHarmonics8BitMode")) >= 0) GL(Uniform1i)(l, u->sh_8bit);
    if ((l = LOC("sphericalHarmonicsMultiTextureMode")) >= 0) GL(Uniform1i)(l, 0);
    if ((l = LOC("fadeInComplete")) >= 0) GL(Uniform1i)(l, u->fade_in_complete);
    if ((l = LOC("sceneCount")) >= 0) GL(Uniform1i)(l, u->scene_count);
    if ((l = LOC("sceneCenter")) >= 0) GL(Uniform3f)(l, u->scene_center[0], u->scene_center[1], u->scene_center[2]);
    if ((l = LOC("visibleRegionFadeStartRadius")) >= 0) GL(Uniform1f)(l, u->fade_start_radius);
    if ((l = LOC("visibleRegionRadius")) >= 0) GL(Uniform1f)(l, 0.0f);
    if ((l = LOC("currentTime")) >= 0) GL(Uniform1f)(l, 0.0f);
    if ((l = LOC("firstRenderTime")) >= 0) GL(Uniform1f)(l, 0.0f);
    if ((l = LOC("sphericalHarmonics8BitCompressionRangeMin")) >= 0) GL(Uniform1fv)(l, 32, u->sh8_min);
    if ((l = LOC("sphericalHarmonics8BitCompressionRangeMax")) >= 0) GL(Uniform1fv)(l, 32, u->sh8_max);
    if ((l = LOC("transforms")) >= 0) GL(UniformMatrix4fv)(l, 32, GL_FALSE, &u->transforms[0][0]);
    if ((l = LOC("sceneOpacity")) >= 0) GL(Uniform1fv)(l, 32, u->scene_opacity);
    if ((l = LOC("sceneVisibility")) >= 0) GL(Uniform1iv)(l, 32, u->scene_visibility);
#undef LOC
}

/* The instanced quad of SplatGeometry.build (:14-37): `position` per vertex, `splatIndex` per instance (uint, divisor 1) */
static GLuint quad_vao(GLuint prog, const uint32_t* splat_index, uint32_t count, GLuint bufs[3]) {
    static const float corners[12] = {-1, -1, 0, -1, 1, 0, 1, 1, 0, 1, -1, 0};
    static const uint16_t index[6] = {0, 1, 2, 0, 2, 3};
    GLuint vao;
    GL(GenVertexArrays)(1, &vao);
    GL(BindVertexArray)(vao);
    GL(GenBuffers)(3, bufs);
    GL(BindBuffer)(GL_ARRAY_BUFFER, bufs[0]);
    GL(BufferData)(GL_ARRAY_BUFFER, sizeof corners, corners, GL_STATIC_DRAW);
    GLint lp = GL(GetAttribLocation)(prog, "position");
    GL(EnableVertexAttribArray)((GLuint)lp);
    GL(VertexAttribPointer)((GLuint)lp, 3, GL_FLOAT, GL_FALSE, 0, 0);
    GL(BindBuffer)(GL_ARRAY_BUFFER, bufs[1]);
    GL(BufferData)(GL_ARRAY_BUFFER, sizeof(uint32_t) * (count ? count : 1), splat_index, GL_STATIC_DRAW);
    GLint li = GL(GetAttribLocation)(prog, "splatIndex");
    GL(EnableVertexAttribArray)((GLuint)li);
    GL(VertexAttribIPointer)((GLuint)li, 1, GL_UNSIGNED_INT, 0, 0);
    GL(VertexAttribDivisor)((GLuint)li, 1);
    GL(BindBuffer)(GL_ELEMENT_ARRAY_BUFFER, bufs[2]);
    GL(BufferData)(GL_ELEMENT_ARRAY_BUFFER, sizeof index, index, GL_STATIC_DRAW);
    return vao;
}

static void release(GLuint prog, GLuint vao, GLuint bufs[3], Textures* t) {
    GL(BindVertexArray)(0);
    GL(DeleteVertexArrays)(1, &vao);
    GL(DeleteBuffers)(3, bufs);
    GL(DeleteTextures)(t->ntex, t->tex);
    GL(UseProgram)(0);
    GL(DeleteProgram)(prog);
}

/* ---------------------------------------------------------------------------------------------------- transform feedback
 * splat_index: the splats to run (NULL: 0 .. count-1 of the scene); out: float [ninst, 4 corners, 10] = gl_Position[4],
 * vColor[4], vPosition[2] per corner in SplatGeometry's order.  GLES 3.0 allows no indexed draw while transform feedback is
 * active, so each instance draws its 4 corners once as GL_POINTS. */
int glref_capture_vertices(const char* vert, const char* frag, const HarnessScene* sc, const HarnessUniforms* u,
                           const uint32_t* splat_index, uint32_t ninst, float* out) {
    GLuint prog = program(vert, frag, 0, 1);
    if (!prog) return -10;
    GL(UseProgram)(prog);
    Textures t;
    if (data_textures(prog, sc, &t)) return -11;
    uniforms(prog, u);
    uint32_t* idx = NULL;
    if (!splat_index) {
        idx = (uint32_t*)malloc(sizeof(uint32_t) * (ninst ? ninst : 1));
        for (uint32_t i = 0; i < ninst; i++) idx[i] = i;
        splat_index = idx;
    }
    GLuint bufs[3], tfb;
    GLuint vao = quad_vao(prog, splat_index, ninst, bufs);
    free(idx);
    const size_t bytes = sizeof(float) * 40 * (size_t)ninst;
    GL(GenBuffers)(1, &tfb);
    GL(BindBuffer)(GL_TRANSFORM_FEEDBACK_BUFFER, tfb);
    GL(BufferData)(GL_TRANSFORM_FEEDBACK_BUFFER, (GLsizeiptr)bytes, NULL, GL_STATIC_READ);
    GL(BindBufferBase)(GL_TRANSFORM_FEEDBACK_BUFFER, 0, tfb);
    GL(Enable)(GL_RASTERIZER_DISCARD);
    GL(BeginTransformFeedback)(GL_POINTS);
    GL(DrawArraysInstanced)(GL_POINTS, 0, 4, (GLsizei)ninst);
    GL(EndTransformFeedback)();
    GL(Disable)(GL_RASTERIZER_DISCARD);
    int rc = gl_check("transform feedback");
    const void* m = GL(MapBufferRange)(GL_TRANSFORM_FEEDBACK_BUFFER, 0, (GLsizeiptr)bytes, GL_MAP_READ_BIT);
    if (m) { memcpy(out, m, bytes); GL(UnmapBuffer)(GL_TRANSFORM_FEEDBACK_BUFFER); } else rc = -12;
    GL(BindBufferBase)(GL_TRANSFORM_FEEDBACK_BUFFER, 0, 0);
    GL(DeleteBuffers)(1, &tfb);
    release(prog, vao, bufs, &t);
    return rc;
}

/* ---------------------------------------------------------------------------------------------------- frames */
typedef struct { GLuint fbo, color, depth; } Target;

static int target(int w, int h, GLenum depth_format, Target* t) {
    GL(GenFramebuffers)(1, &t->fbo);
    GL(BindFramebuffer)(GL_FRAMEBUFFER, t->fbo);
    GL(GenRenderbuffers)(1, &t->color);
    GL(BindRenderbuffer)(GL_RENDERBUFFER, t->color);
    GL(RenderbufferStorage)(GL_RENDERBUFFER, GL_RGBA8, w, h);
    GL(FramebufferRenderbuffer)(GL_FRAMEBUFFER, GL_COLOR_ATTACHMENT0, GL_RENDERBUFFER, t->color);
    GL(GenRenderbuffers)(1, &t->depth);
    GL(BindRenderbuffer)(GL_RENDERBUFFER, t->depth);
    GL(RenderbufferStorage)(GL_RENDERBUFFER, depth_format, w, h);
    GL(FramebufferRenderbuffer)(GL_FRAMEBUFFER, GL_DEPTH_ATTACHMENT, GL_RENDERBUFFER, t->depth);
    GLenum st = GL(CheckFramebufferStatus)(GL_FRAMEBUFFER);
    if (st != GL_FRAMEBUFFER_COMPLETE) { fprintf(stderr, "gl_ref: FBO incomplete 0x%04x\n", st); return -20; }
    GL(Viewport)(0, 0, w, h);
    return gl_check("target");
}

static void target_release(Target* t) {
    GL(BindFramebuffer)(GL_FRAMEBUFFER, 0);
    GL(DeleteRenderbuffers)(1, &t->color);
    GL(DeleteRenderbuffers)(1, &t->depth);
    GL(DeleteFramebuffers)(1, &t->fbo);
}

/* What the host's own geometry left before the splats are drawn: depth and colour written per pixel from textures (our own
 * program: a full-screen triangle pair; gl_FragDepth goes through the depth buffer's own format conversion). */
static const char* DST_VS =
    "#version 300 es\nin vec2 p;\nvoid main() { gl_Position = vec4(p, 0.0, 1.0); }\n";
static const char* DST_FS =
    "#version 300 es\nprecision highp float;\nuniform highp sampler2D d;\nuniform highp sampler2D c;\n"
    "layout(location = 0) out highp vec4 o;\n"
    "void main() { ivec2 q = ivec2(gl_FragCoord.xy); gl_FragDepth = texelFetch(d, q, 0).r; o = texelFetch(c, q, 0); }\n";

static int destination(int w, int h, const float* dst_depth, const uint8_t* dst_rgba) {
    static const uint8_t clear_rgba[4] = {0, 0, 0, 0};
    GLuint prog = program(DST_VS, DST_FS, 1, 0);
    if (!prog) return -21;
    GL(UseProgram)(prog);
    GLuint tex[2], buf, vao;
    tex[0] = upload(0, GL_R32F, w, h, GL_RED, GL_FLOAT, dst_depth);
    uint8_t* c = NULL;
    if (!dst_rgba) {
        c = (uint8_t*)malloc(4 * (size_t)w * h);
        for (size_t i = 0; i < (size_t)w * h; i++) memcpy(c + 4 * i, clear_rgba, 4);
    }
    tex[1] = upload(1, GL_RGBA8, w, h, GL_RGBA, GL_UNSIGNED_BYTE, dst_rgba ? (const void*)dst_rgba : (const void*)c);
    free(c);
    set_sampler(prog, "d", 0);
    set_sampler(prog, "c", 1);
    static const float tri[12] = {-1, -1, 1, -1, 1, 1, -1, -1, 1, 1, -1, 1};
    GL(GenVertexArrays)(1, &vao);
    GL(BindVertexArray)(vao);
    GL(GenBuffers)(1, &buf);
    GL(BindBuffer)(GL_ARRAY_BUFFER, buf);
    GL(BufferData)(GL_ARRAY_BUFFER, sizeof tri, tri, GL_STATIC_DRAW);
    GLint lp = GL(GetAttribLocation)(prog, "p");
    GL(EnableVertexAttribArray)((GLuint)lp);
    GL(VertexAttribPointer)((GLuint)lp, 2, GL_FLOAT, GL_FALSE, 0, 0);
    GL(Enable)(GL_DEPTH_TEST);
    GL(DepthFunc)(GL_ALWAYS);
    GL(DepthMask)(GL_TRUE);
    GL(Disable)(GL_BLEND);
    GL(DrawArrays)(GL_TRIANGLES, 0, 6);
    int rc = gl_check("destination");
    GL(BindVertexArray)(0);
    GL(DeleteVertexArrays)(1, &vao);
    GL(DeleteBuffers)(1, &buf);
    GL(DeleteTextures)(2, tex);
    GL(UseProgram)(0);
    GL(DeleteProgram)(prog);
    return rc;
}

/* One frame: clear to (0,0,0,0) (depth 1), the destination if given (dst_depth: float [h, w] window depth, row 0 = bottom;
 * dst_rgba: uint8 [h, w, 4] or NULL for the clear colour), then ONE glDrawElementsInstanced of the quad over `order` with the
 * material state of SplatMaterial3D.js:65-75 as three r160 applies it: NormalBlending = blend equation ADD,
 * blendFuncSeparate(SRC_ALPHA, ONE_MINUS_SRC_ALPHA, ONE, ONE_MINUS_SRC_ALPHA); depthTest on (LessEqualDepth), depthWrite off;
 * side DoubleSide = no culling.  depth_format: 0 DEPTH_COMPONENT32F, 1 DEPTH_COMPONENT24.  out_rgba8: [h, w, 4], row 0 = bottom. */
int glref_draw_frame(const char* vert, const char* frag, const HarnessScene* sc, const HarnessUniforms* u, const uint32_t* order,
                     uint32_t count, int w, int h, const float* dst_depth, int depth_format, const uint8_t* dst_rgba,
                     uint8_t* out_rgba8) {
    Target tg;
    int rc = target(w, h, depth_format ? GL_DEPTH_COMPONENT24 : GL_DEPTH_COMPONENT32F, &tg);
    if (rc) return rc;
    GL(ColorMask)(GL_TRUE, GL_TRUE, GL_TRUE, GL_TRUE);
    GL(DepthMask)(GL_TRUE);
    GL(ClearColor)(0.0f, 0.0f, 0.0f, 0.0f);
    GL(ClearDepthf)(1.0f);
    GL(Clear)(GL_COLOR_BUFFER_BIT | GL_DEPTH_BUFFER_BIT);
    if (dst_depth && (rc = destination(w, h, dst_depth, dst_rgba))) return rc;
    GLuint prog = program(vert, frag, 0, 0);
    if (!prog) return -22;
    GL(UseProgram)(prog);
    Textures t;
    if (data_textures(prog, sc, &t)) return -23;
    uniforms(prog, u);
    GLuint bufs[3];
    GLuint vao = quad_vao(prog, order, count, bufs);
    GL(Disable)(GL_CULL_FACE);
    GL(Enable)(GL_DEPTH_TEST);
    GL(DepthFunc)(GL_LEQUAL);
    GL(DepthMask)(GL_FALSE);
    GL(Enable)(GL_BLEND);
    GL(BlendEquation)(GL_FUNC_ADD);
    GL(BlendFuncSeparate)(GL_SRC_ALPHA, GL_ONE_MINUS_SRC_ALPHA, GL_ONE, GL_ONE_MINUS_SRC_ALPHA);
    GL(DrawElementsInstanced)(GL_TRIANGLES, 6, GL_UNSIGNED_SHORT, 0, (GLsizei)count);
    rc = gl_check("draw");
    GL(PixelStorei)(GL_PACK_ALIGNMENT, 1);
    GL(ReadPixels)(0, 0, w, h, GL_RGBA, GL_UNSIGNED_BYTE, out_rgba8);
    if (!rc) rc = gl_check("readpixels");
    GL(Disable)(GL_BLEND);
    GL(Disable)(GL_DEPTH_TEST);
    release(prog, vao, bufs, &t);
    target_release(&tg);
    return rc;
}

/* ---------------------------------------------------------------------------------------------------- fragment samples
 * The reference's fragment shader at given varyings: each sample is one 1-pixel point into a count x 1 RGBA32F target (no blend),
 * drawn by our own vertex shader that passes vColor / vPosition through flat.  Discarded samples keep the clear value, whose
 * alpha (-1) no fragment can write. */
static const char* FS_PROBE_VS =
    "#version 300 es\nin vec2 vp;\nin vec4 vc;\nflat out vec4 vColor;\nflat out vec2 vPosition;\nuniform float n;\n"
    "void main() { vColor = vc; vPosition = vp; gl_PointSize = 1.0;\n"
    "  gl_Position = vec4((float(gl_VertexID) + 0.5) / n * 2.0 - 1.0, 0.0, 0.0, 1.0); }\n";

int glref_run_fragment(const char* frag, uint32_t count, const float* v_position, const float* v_color, float* out_rgba,
                       uint8_t* out_discard) {
    /* The varyings of the reference's fragment shader are plain (smooth) `in`s; the probe's are flat.  GLSL ES 3.00 requires
     * matching interpolation qualifiers, so the reference's `varying` is declared flat by the define below: for a single
     * point every qualifier yields the provoking vertex's value, so no value changes. */
    char* f = three_prefix(frag, 1);
    const char* v1 = "#define varying in\n";
    char* p = strstr(f, v1);
    if (!p) { free(f); return -30; }
    const char* v2 = "#define varying flat in\n";
    char* g = (char*)malloc(strlen(f) + 16);
    memcpy(g, f, (size_t)(p - f));
    strcpy(g + (p - f), v2);
    strcat(g, p + strlen(v1));
    free(f);
    GLuint prog = program(FS_PROBE_VS, g, 1, 0);
    free(g);
    if (!prog) return -31;
    GL(UseProgram)(prog);
    GLint l = GL(GetUniformLocation)(prog, "n");
    GL(Uniform1f)(l, (float)count);
    GLuint fbo, rb, vao, buf[2];
    GL(GenFramebuffers)(1, &fbo);
    GL(BindFramebuffer)(GL_FRAMEBUFFER, fbo);
    GL(GenRenderbuffers)(1, &rb);
    GL(BindRenderbuffer)(GL_RENDERBUFFER, rb);
    GL(RenderbufferStorage)(GL_RENDERBUFFER, GL_RGBA32F, (GLsizei)count, 1);
    GL(FramebufferRenderbuffer)(GL_FRAMEBUFFER, GL_COLOR_ATTACHMENT0, GL_RENDERBUFFER, rb);
    if (GL(CheckFramebufferStatus)(GL_FRAMEBUFFER) != GL_FRAMEBUFFER_COMPLETE) { fprintf(stderr, "gl_ref: RGBA32F target incomplete\n"); return -32; }
    GL(Viewport)(0, 0, (GLsizei)count, 1);
    GL(Disable)(GL_BLEND);
    GL(Disable)(GL_DEPTH_TEST);
    GL(ClearColor)(0.0f, 0.0f, 0.0f, -1.0f);
    GL(Clear)(GL_COLOR_BUFFER_BIT);
    GL(GenVertexArrays)(1, &vao);
    GL(BindVertexArray)(vao);
    GL(GenBuffers)(2, buf);
    GL(BindBuffer)(GL_ARRAY_BUFFER, buf[0]);
    GL(BufferData)(GL_ARRAY_BUFFER, sizeof(float) * 2 * count, v_position, GL_STATIC_DRAW);
    GLint lp = GL(GetAttribLocation)(prog, "vp");
    GL(EnableVertexAttribArray)((GLuint)lp);
    GL(VertexAttribPointer)((GLuint)lp, 2, GL_FLOAT, GL_FALSE, 0, 0);
    GL(BindBuffer)(GL_ARRAY_BUFFER, buf[1]);
    GL(BufferData)(GL_ARRAY_BUFFER, sizeof(float) * 4 * count, v_color, GL_STATIC_DRAW);
    GLint lc = GL(GetAttribLocation)(prog, "vc");
    GL(EnableVertexAttribArray)((GLuint)lc);
    GL(VertexAttribPointer)((GLuint)lc, 4, GL_FLOAT, GL_FALSE, 0, 0);
    GL(DrawArrays)(GL_POINTS, 0, (GLsizei)count);
    int rc = gl_check("fragment samples");
    GL(PixelStorei)(GL_PACK_ALIGNMENT, 1);
    GL(ReadPixels)(0, 0, (GLsizei)count, 1, GL_RGBA, GL_FLOAT, out_rgba);
    if (!rc) rc = gl_check("fragment readpixels");
    for (uint32_t i = 0; i < count; i++) out_discard[i] = out_rgba[4 * i + 3] == -1.0f;
    GL(BindVertexArray)(0);
    GL(DeleteVertexArrays)(1, &vao);
    GL(DeleteBuffers)(2, buf);
    GL(BindFramebuffer)(GL_FRAMEBUFFER, 0);
    GL(DeleteRenderbuffers)(1, &rb);
    GL(DeleteFramebuffers)(1, &fbo);
    GL(UseProgram)(0);
    GL(DeleteProgram)(prog);
    return rc;
}
