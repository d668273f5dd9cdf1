/* tests/tools/gl_surfel.c — TEST INFRASTRUCTURE: the headless GLES 3 harness (Mesa llvmpipe, oracle/gl_ref.c) for the reference's
 * SplatMaterial2D strings.  Built into oracle/_ref/ by tests/tools/make_surfel_golden.py, never by build().
 *
 * The scene arrives as oracle/gl_ref.c's HarnessScene with the six values per splat of 2D mode - scale x, y, z, rotation x, y, z -
 * in `cov`: SplatMesh packs them exactly as the fp32 covariance texture (4 elements per texel, 6 per splat; SplatMesh.js:763-786),
 * so gl_ref.c's upload is the right one and only the sampler's name differs (scaleRotationsTexture / ...Size on the same unit). */
#include "../../oracle/gl_ref.c"

static void bind_scale_rotations(GLuint prog, const HarnessScene* sc) {
    int w, h;
    ref_size(4, 6, sc->count, &w, &h);
    set_sampler(prog, "scaleRotationsTexture", 1);
    set_size(prog, "scaleRotationsTextureSize", w, h);
}

/* transform feedback of gl_Position (4), vColor (4), vT (9, column by column), vQuadCenter (2), vFragCoord (2) = 21 floats for every
 * (splat, quad corner), corners in SplatGeometry's order; out: float [ninst, 4, 21] */
int glsurfel_capture_vertices(const char* vert, const char* frag, const HarnessScene* sc, const HarnessUniforms* u, uint32_t ninst,
                              float* out) {
    char* v = three_prefix(vert, 0);
    char* f = three_prefix(frag, 1);
    GLuint vs = compile(GL_VERTEX_SHADER, v), fs = compile(GL_FRAGMENT_SHADER, f);
    free(v); free(f);
    if (!vs || !fs) return -10;
    GLuint prog = GL(CreateProgram)();
    GL(AttachShader)(prog, vs);
    GL(AttachShader)(prog, fs);
    const char* names[] = {"gl_Position", "vColor", "vT", "vQuadCenter", "vFragCoord"};
    GL(TransformFeedbackVaryings)(prog, 5, names, GL_INTERLEAVED_ATTRIBS);
    GL(LinkProgram)(prog);
    GL(DeleteShader)(vs);
    GL(DeleteShader)(fs);
    GLint ok = 0;
    GL(GetProgramiv)(prog, GL_LINK_STATUS, &ok);
    if (!ok) {
        char log[4096];
        GL(GetProgramInfoLog)(prog, sizeof log, NULL, log);
        fprintf(stderr, "gl_surfel: link: %s\n", log);
        return -10;
    }
    GL(UseProgram)(prog);
    Textures t;
    if (data_textures(prog, sc, &t)) return -11;
    bind_scale_rotations(prog, sc);
    uniforms(prog, u);
    uint32_t* idx = (uint32_t*)malloc(sizeof(uint32_t) * (ninst ? ninst : 1));
    for (uint32_t i = 0; i < ninst; i++) idx[i] = i;
    GLuint bufs[3], tfb;
    GLuint vao = quad_vao(prog, idx, ninst, bufs);
    free(idx);
    const size_t bytes = sizeof(float) * 84 * (size_t)ninst;
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

/* One frame with the material's state (SplatMaterial2D.js:45-55: NormalBlending, depthTest, no depth write, DoubleSide) into an
 * RGBA8 target, as oracle/gl_ref.c's glref_draw_frame draws the 3D material; arguments as there. */
int glsurfel_draw_frame(const char* vert, const char* frag, const HarnessScene* sc, const HarnessUniforms* u, const uint32_t* order,
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
    bind_scale_rotations(prog, sc);
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
