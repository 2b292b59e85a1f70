/*
 * eigen_engine.h -- C ABI of the MI355X (gfx950) fitness-evaluation engine for EIGen.
 *
 * Drop-in boundary for ONE hot path of LanaSina/evolutionary_illusion_generator: per genome
 *   CPPN render -> PredNet roll-out (20 repeats + self-fed frames) -> Lucas-Kanade flow -> motion score.
 * The reference is pure Python and has no FFI; each entry point below replaces the Python-level call the
 * reference makes at the cited file:line, and is what a ctypes binding on the reference side would bind
 * (stub shown in INTEGRATION.md).  Plain pointers and sizes only; no C++/torch types.
 *
 * Conventions
 *   - every function returns 0 on success or a negative eigen_status; eigen_last_error() gives the text
 *     (thread-local);  no exception crosses the ABI.
 *   - pointers named h_* are HOST memory, d_* are DEVICE (HIP) memory on the engine's device.  The caller
 *     owns all of them; the engine owns only its handle and its internal device workspaces.
 *   - all device work is enqueued on the caller-supplied hipStream_t (passed as void*; NULL = default
 *     stream).  Functions that return host results (h_* outputs) synchronise that stream before returning.
 *   - a handle is not thread-safe; use one handle per process/rank (one rank per GPU).
 *   - images are PLANAR uint8 [B][C][H][W] (C = 1 gray or 3 RGB), the CHW form the reference feeds PredNet.
 */
#ifndef EIGEN_ENGINE_H
#define EIGEN_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EIGEN_MAX_LAYERS 8
#define EIGEN_ABI_VERSION 4 /* 2: eigen_config grew (flow_method, fb_*), eigen_debug_dense_flow, gradient = 2; 3: eigen_gate_order; 4: eigen_winograd_mask */

typedef enum {
    EIGEN_OK = 0,
    EIGEN_ERR_INVALID = -1,   /* bad argument / unsupported configuration */
    EIGEN_ERR_HIP = -2,       /* HIP runtime error (message has the hipError string) */
    EIGEN_ERR_STATE = -3,     /* call order: weights / grid not set */
    EIGEN_ERR_CAPACITY = -4   /* batch, genome or feature count exceeds what the handle was created for */
} eigen_status;

/* StructureType of the reference (generate_illusion.py:25-29, fitness_calculator.py:10-14) */
typedef enum { EIGEN_BANDS = 0, EIGEN_CIRCLES = 1, EIGEN_FREE = 2, EIGEN_CIRCLES_FREE = 3 } eigen_structure;
/* eigen_score only: inside_outside_score(vectors, width, height) (fitness_calculator.py:219-304) on ALL the given vectors.
 * The reference reaches it only through an else branch that raises NameError (generate_illusion.py:606-607,
 * fitness_calculator.py:545-546), so no structure selects it on the population path. */
#define EIGEN_SCORE_INSIDE_OUTSIDE 4

/* Which two frames Lucas-Kanade compares:
 *   POPULATION: prediction after step n_repeat -> first extension frame   (generate_illusion.py:543-550)
 *   SINGLE    : the input image -> second extension frame                 (fitness_calculator.py:493-498) */
typedef enum { EIGEN_PAIR_POPULATION = 0, EIGEN_PAIR_SINGLE = 1 } eigen_pairing;

/* CPPN activation ids (PyTorch-NEAT activations.py; neat_configs/ circles.txt:12 lists the options in use) */
typedef enum {
    EIGEN_ACT_SIGMOID = 0, /* 1/(1+exp(-5x)) */
    EIGEN_ACT_TANH = 1,    /* tanh(2.5x)     */
    EIGEN_ACT_ABS = 2,
    EIGEN_ACT_GAUSS = 3,   /* exp(-5x^2)     */
    EIGEN_ACT_IDENTITY = 4,
    EIGEN_ACT_SIN = 5,
    EIGEN_ACT_RELU = 6
} eigen_activation;

typedef struct {
    int32_t device;                        /* HIP device ordinal */
    int32_t width, height;                 /* image size; both divisible by 2^(n_layers-1) */
    int32_t n_layers;
    int32_t channels[EIGEN_MAX_LAYERS];    /* PredNet channels, channels[0] = c_dim (1 or 3) */
    int32_t max_batch;                     /* genomes evaluated per device batch (workspace sizing) */
    /* constants hard-coded in the reference (generate_illusion.py:482,531; fitness_calculator.py:470-471) */
    int32_t n_repeat;                      /* 20 */
    int32_t n_ext;                         /* 2  */
    int32_t requant_feedback;              /* 0: extension frames feed the float prediction back (upstream) */
    /* Optical_Flow_Analyzer / OpenCV parameters (goodFeaturesToTrack, calcOpticalFlowPyrLK) */
    int32_t lk_max_corners;                /* 100  (<= 128) */
    int32_t lk_block_size;                 /* 7    */
    int32_t lk_win;                        /* 15   */
    int32_t lk_max_level;                  /* 2    */
    int32_t lk_max_iter;                   /* 10   */
    int32_t flow_method;                   /* EIGEN_FLOW_LK (0, what the reference calls) or EIGEN_FLOW_FARNEBACK (1) */
    double lk_quality_level;               /* 0.3  */
    double lk_min_distance;                /* 7    */
    double lk_epsilon;                     /* 0.03 */
    double lk_min_eig_thr;                 /* 1e-4 */
    /* Dense flow after Farneback, cv::calcOpticalFlowFarneback with the parameters of OpenCV's dense-flow tutorial
     * (pyr_scale is fixed at 0.5).  The reference never calls a dense-flow routine (its only flow call is lucas_kanade,
     * generate_illusion.py:549-550); the option answers the north star's "Farneback/Lucas-Kanade flow".  The dense field is
     * sampled every fb_step pixels from fb_step/2 (the grid of OpenCV's samples/python/opt_flow.py; the step grows by
     * multiples of fb_step until the grid fits lk_max_corners vectors) into the same [x, y, dx, dy] vectors. */
    int32_t fb_levels;                     /* 3  (levels on top of the full resolution; fewer if a level would be < 32 px) */
    int32_t fb_winsize;                    /* 15 (odd, <= 33) */
    int32_t fb_iterations;                 /* 3  */
    int32_t fb_poly_n;                     /* 5  (<= 7) */
    int32_t fb_step;                       /* 16 */
    int32_t reserved1;
    double fb_poly_sigma;                  /* 1.2 */
} eigen_config;

typedef enum { EIGEN_FLOW_LK = 0, EIGEN_FLOW_FARNEBACK = 1 } eigen_flow_method;

/* A batch of CPPN genomes, flattened by the host (create_cppn semantics, generate_illusion.py:384-389):
 * per genome g, nodes node_off[g]..node_off[g+1]-1 are in topological order; node n has incoming edges
 * edge_off[n]..edge_off[n+1]-1 (global edge index), summed left to right in that order;
 * value(n) = act(response * sum_k(weight_k * value(src_k)) + bias).
 * edge_src >= 0 : index of a node of the same genome (relative to node_off[g]);
 * edge_src <  0 : leaf plane  -1 -> plane 0 (x), -2 -> plane 1 (y), ...; -(n_planes+1) -> the constant 1.0.
 * out_node[g*c_out + c]: node (relative index) rendered into channel c. */
typedef struct {
    int32_t n_genomes;
    int32_t c_out;              /* outputs rendered per genome: c_dim, or 1 when gradient == 0 */
    const int32_t* node_off;    /* [n_genomes + 1] */
    const int32_t* edge_off;    /* [total_nodes + 1] */
    const uint8_t* node_act;    /* [total_nodes] eigen_activation */
    const double* node_bias;    /* [total_nodes] */
    const double* node_resp;    /* [total_nodes] */
    const int32_t* edge_src;    /* [total_edges] */
    const double* edge_w;       /* [total_edges] */
    const int32_t* out_node;    /* [n_genomes * c_out] */
} eigen_genome_batch;

typedef struct eigen_engine eigen_engine;

int eigen_abi_version(void);
const char* eigen_last_error(void);

/* Defaults = the constants of the reference + OpenCV tutorial LK parameters; fills every field but
 * device/width/height/n_layers/channels/max_batch. */
void eigen_config_defaults(eigen_config* cfg);

int eigen_create(const eigen_config* cfg, eigen_engine** out);
int eigen_destroy(eigen_engine* e);

/* Replaces `serializers.load_npz(initmodel, model)` inside test_prednet (generate_illusion.py:533).
 * h_tensors: host float32 tensors in the order of evolutionary_illusion_generator_amd.weights.tensor_names()
 * (per layer: [ConvA W,b (l>0)], ConvP W,b, per gate i,f,c,o: x0 W, [x1 W], h W, h b; peepholes c_i,c_f,c_o). */
int eigen_set_prednet_weights(eigen_engine* e, const float* const* h_tensors, int32_t n_tensors);

/* Replaces the per-generation create_grid result (generate_illusion.py:501) as consumed by
 * get_image_from_cppn (:375-378): n_planes float64 planes of H*W values; background where plane 0 == -1. */
int eigen_set_grid(eigen_engine* e, const double* h_planes, int32_t n_planes);

/* Replaces get_image_from_cppn (generate_illusion.py:372-460) for a whole batch.
 * d_images: uint8 [n_genomes][c_dim][H][W].  bg: 1 white / 0 black.  gradient: 1 / 0 as in the reference's
 * get_image_from_cppn (generate_illusion.py:372-460); 2 = get_equilum_image_from_cppn (:333-367, c_dim 3): the three
 * output nodes are h, s, v, converted per pixel as colorsys.hsv_to_rgb does, bg applied to h, s and v beforehand. */
int eigen_render_cppn(eigen_engine* e, const eigen_genome_batch* h_genomes, int32_t bg, int32_t gradient,
                      uint8_t* d_images, void* stream);

/* Replaces the node calls `node_func(x=inp_x, y=inp_y)` on the objects create_cppn returns (PyTorch-NEAT
 * Node.__call__; generate_illusion.py:395, 406, 443) for a batch: the raw float64 value of every output node
 * at every pixel of the planes given to eigen_set_grid, no background fill and no quantisation.
 * d_nodes: float64 [n_genomes][c_out][H*W].  Used by the import shim pytorch_neat.pytorch_neat.cppn. */
int eigen_eval_cppn_nodes(eigen_engine* e, const eigen_genome_batch* h_genomes, double* d_nodes, void* stream);

/* Moving CPPN textures with their exact flow ("Moving textures"): n sequences of n_frames frames, each the
 * gradient = 1 render of one or two genomes on affine coordinates.  Genome b * n_layers + l of the batch is layer l of sample b.
 *   px = col - (W - 1) / 2, py = row - (H - 1) / 2; with A = h_affine[b][t][l] (pixel -> texture):
 *   u = (a0 px + a1 py) + a2, v = (a3 px + a4 py) + a5, every product and sum one float64 rounding; leaves x = u, y = v, any further
 *   leaf reads 1.0.  Layer 0 covers every pixel, layer 1 where u1 u1 + v1 v1 < 1.0 (a unit disc in its texture space); a pixel shows
 *   the topmost layer that covers it.  byte = uint8(255 value_c) of the visible layer's output c, as eigen_render_cppn's gradient = 1
 *   render quantises, with no background fill: a coordinate of exactly -1.0 is an ordinary coordinate.
 *   d_frames: uint8, sample b at d_frames + b * f_bstride as [n_frames][c_dim][H][W]; f_bstride >= n_frames*C*H*W, the bytes between
 *     two samples are not written.
 *   d_flow (or NULL): float64 [n][n_frames - 1][2][H][W].  With I = h_affine_inv[b][t + 1][visible layer] (texture -> pixel centre)
 *     slot t holds ((i0 u + i1 v) + i2 - px, (i3 u + i4 v) + i5 - py): where the surface visible at the pixel in frame t is in frame
 *     t + 1, whether or not it is visible there.  The inverses are the caller's: nothing is inverted here.
 *   d_layer (or NULL): uint8 [n][n_frames][H][W], the visible layer, 0 or 1.
 * The entry needs neither a grid nor weights, reads no kept sequence state and uses no workspace of the handle but the genome staging
 * buffers, which grow with the call: n is not tied to max_batch.  One sample is one row of the launch, hence n <= 65535.
 * Errors, before anything is launched or allocated: EIGEN_ERR_INVALID a NULL handle, batch, h_affine or d_frames, n_layers outside
 * 1 .. 2, n_frames < 1, n < 1, d_flow with n_frames < 2, d_flow without h_affine_inv or h_affine_inv without d_flow, n_genomes !=
 * n * n_layers, c_out < c_dim, f_bstride < n_frames*C*H*W, and the genome checks of eigen_render_cppn (against two leaf planes);
 * EIGEN_ERR_CAPACITY n > 65535, or a sample whose larger program's node values, beside both programs, need more than 160 KiB of LDS. */
int eigen_render_moving_cppn(eigen_engine* e, const eigen_genome_batch* h_genomes, int32_t n, int32_t n_frames, int32_t n_layers,
                             const double* h_affine,      /* [n][n_frames][n_layers][6] pixel -> texture */
                             const double* h_affine_inv,  /* same shape, texture -> pixel; NULL iff d_flow is NULL */
                             uint8_t* d_frames, int64_t f_bstride,
                             double* d_flow, uint8_t* d_layer, void* stream);

/* The validity planes of eigen_render_moving_cppn's flow ("The joint objective and the valid pixels"): whether
 * the surface a pixel of frame t shows can be seen in frame t + 1.  From the affines alone, in the render's arithmetic (float64, every
 * product and sum one rounding in the order written); no genome is read.  With (u, v) and the visible layer vis of the pixel in frame
 * t as the render forms them and I = h_affine_inv[b][t + 1][vis]:
 *   qx = (i0 u + i1 v) + i2, qy = (i3 u + i4 v) + i5            (the render's flow is (qx - px, qy - py))
 *   inb = -(W - 1) / 2 <= qx <= (W - 1) / 2 && -(H - 1) / 2 <= qy <= (H - 1) / 2
 *   occ = n_layers == 2 && vis == 0 && u1' u1' + v1' v1' < 1.0, (u1', v1') = h_affine[b][t + 1][1] applied to (qx, qy)
 *   valid = inb && !occ, a byte 0 or 1; a NaN compares false and gives 0.
 * h_affine, h_affine_inv: [n][n_frames][n_layers][6], as eigen_render_moving_cppn takes them.  d_valid: uint8 [n][n_frames - 1][H][W].
 * The entry needs neither a grid nor weights and uses staging buffers of its own, which grow with the call.
 * Errors, before anything is launched or allocated: EIGEN_ERR_INVALID a NULL handle, h_affine, h_affine_inv or d_valid, n_layers
 * outside 1 .. 2, n_frames < 2, n < 1; EIGEN_ERR_CAPACITY n > 65535. */
int eigen_moving_cppn_valid(eigen_engine* e, int32_t n, int32_t n_frames, int32_t n_layers, const double* h_affine,
                            const double* h_affine_inv, uint8_t* d_valid, void* stream);

/* The backward pass through eigen_render_cppn's gradient = 1 render ("CPPN parameter gradients"): the gradient
 * of a loss by every bias, response and connection weight of the batch, from its gradient by the images.
 *   d_image_grad: device float, d loss / d (byte / 255) of image g at d_image_grad + g * g_bstride as [c_dim][H][W] (what
 *     eigen_trainer_loss_grad_frames returns); g_bstride in floats, >= C*H*W; floats between the images are never read.
 *   The forward is the render's arithmetic, so the node values are the render's bits.  The gradient passes straight through the
 *   uint8 quantisation where the byte follows the node: the pixel is not background (plane 0 != -1) and t = trunc(255 v) lies in
 *   [0, 255].  Elsewhere (the fill, the low-byte wrap, NaN) the seed is zero.  bg does not enter the result.
 *   h_grad_bias [total_nodes], h_grad_resp [total_nodes], h_grad_w [total_edges]: host float64, in the batch's own layout, valid on
 *   return (the call synchronises the stream).  An edge from the constant-1 leaf gets its gradient like any other.
 *   The pixels are summed in a fixed order without atomics: two calls give the same bits, and the bits of a genome do not depend on
 *   the batch it is in or on its place in it.
 * Errors: EIGEN_ERR_STATE no grid; EIGEN_ERR_INVALID gradient != 1 (the palette, the rounded gray and the h,s,v renderer are not
 * differentiable here), a NULL pointer, g_bstride < C*H*W, and the genome checks of eigen_render_cppn; EIGEN_ERR_CAPACITY a genome
 * whose node values and adjoints need more than 160 KiB of LDS. */
int eigen_cppn_param_grads(eigen_engine* e, const eigen_genome_batch* h_genomes, int32_t bg, int32_t gradient,
                           const float* d_image_grad, int64_t g_bstride,
                           double* h_grad_bias, double* h_grad_resp, double* h_grad_w, void* stream);

/* Replaces test_prednet (generate_illusion.py:533-537, fitness_calculator.py:487-491) for a batch: state
 * reset, n_repeat steps on the constant frame, then extension steps feeding the prediction back; runs
 * n_steps <= n_repeat + n_ext steps in total.  The quantised prediction of every step t >= first_out_step
 * is written to d_frames[b][t - first_out_step] (uint8 [B][n_steps - first_out_step][C][H][W]). */
int eigen_prednet_rollout(eigen_engine* e, const uint8_t* d_images, int32_t batch, int32_t n_steps,
                          int32_t first_out_step, uint8_t* d_frames, void* stream);

/* PredNet over frame sequences: one step per input frame, then n_ext self-fed steps (cfg.requant_feedback, as in
 * eigen_prednet_rollout).  The arithmetic of every step is the constant-image roll-out's; the first input is frame 0.
 *   d_in: uint8 frames, frame t of sequence b at d_in + b * in_bstride + t * C*H*W (bytes); may be NULL when n_in == 0.
 *   reset = 1: start from reset_state() (needs n_in >= 1).  reset = 0: continue from the state the previous
 *   eigen_prednet_sequence call on this handle left, which must have had the same batch; a roll-out or evaluation on the
 *   handle (eigen_prednet_rollout, eigen_eval_images, eigen_eval_population) discards that state (EIGEN_ERR_STATE).
 *   A sequence run in pieces gives the bytes of one call over the whole sequence.
 *   The quantised prediction of every step t >= first_out_step of THIS call (t counted from 0 in each call) is written
 *   to d_out[b][t - first_out_step] (uint8 [batch][n_in + n_ext - first_out_step][C][H][W]).
 * The number of steps is not bounded by cfg.n_repeat + cfg.n_ext. */
int eigen_prednet_sequence(eigen_engine* e, const uint8_t* d_in, int64_t in_bstride, int32_t batch, int32_t n_in,
                           int32_t n_ext, int32_t reset, int32_t first_out_step, uint8_t* d_out, void* stream);

/* Replaces lucas_kanade (generate_illusion.py:549-550, fitness_calculator.py:498) for a batch of pairs.
 * d_img0/d_img1: uint8 planar images, image b at d_imgX + b * strideX (bytes).
 * d_vectors: float [batch][lk_max_corners][4] rows [x, y, dx, dy]; d_counts: int32 [batch]. */
int eigen_flow(eigen_engine* e, const uint8_t* d_img0, int64_t stride0, const uint8_t* d_img1, int64_t stride1,
               int32_t batch, float* d_vectors, int32_t* d_counts, void* stream);

/* Replaces the scoring block of get_fitnesses_neat (generate_illusion.py:559-616; scorers
 * fitness_calculator.py:18-215).  count == 0 -> the sentinel [[0,0,-1000,0]] -> fitness 0.
 * width/height: the image size the scorers are given (w, h); 0 = the engine's own size.
 * structure EIGEN_SCORE_INSIDE_OUTSIDE: inside_outside_score of the raw vectors (no filter, no sentinel). */
int eigen_score(eigen_engine* e, int32_t structure, int32_t width, int32_t height, const float* d_vectors,
                const int32_t* d_counts, int32_t batch, double* d_fitness, void* stream);

/* The whole path for one batch of genomes: render -> roll-out -> flow -> score.  h_fitness: host double[B].
 * This is what eval_genomes / get_fitnesses_neat (generate_illusion.py:478-673, 692-694) calls per shard. */
int eigen_eval_population(eigen_engine* e, const eigen_genome_batch* h_genomes, int32_t structure, int32_t bg,
                          int32_t gradient, int32_t pairing, double* h_fitness, void* stream);

/* Same, for ready-made images (single-image API, fitness_calculator.py:468-548). */
int eigen_eval_images(eigen_engine* e, const uint8_t* d_images, int32_t batch, int32_t structure,
                      int32_t pairing, double* h_fitness, float* h_vectors, int32_t* h_counts, void* stream);

/* ---- kernel-level entry points used by the parity tests and bench.py's roofline leg ---- */

/* One fused 3x3 convolution chain on the MFMA kernel: out[b][o][y][x] = sum over sources/channels/taps, raw
 * accumulators (no bias).  d_src[i]: float [batch][cin[i]][H>>up[i]][W>>up[i]]; h_w[i]: host float
 * [cout][cin[i]][3][3].  d_out: float [batch][cout][H][W]. */
int eigen_test_conv(eigen_engine* e, int32_t n_src, const float* const* d_src, const int32_t* cin,
                    const int32_t* up, const float* const* h_w, int32_t cout, int32_t H, int32_t W,
                    int32_t batch, float* d_out, void* stream);

/* eigen_test_conv's launch repeated `iters` times between two HIP events on the launch stream; *h_ms = average
 * kernel duration in milliseconds (measurement hook of scripts/ and bench.py). */
int eigen_time_conv(eigen_engine* e, int32_t n_src, const float* const* d_src, const int32_t* cin, const int32_t* up,
                    const float* const* h_w, int32_t cout, int32_t H, int32_t W, int32_t batch, float* d_out,
                    int32_t iters, double* h_ms, void* stream);

/* Host-side helper (no device work): flattens a batch of NEAT genomes, given as plain arrays, into the arrays behind
 * eigen_genome_batch -- the graph part of what PyTorch-NEAT's create_cppn does for the reference
 * (generate_illusion.py:384-389: which connections are expressed, evaluation order, constant nodes).  It is the C twin of
 * evolutionary_illusion_generator_amd/genome.py: _flatten_lists (same output, element for element; tests/test_host_logic.py).
 *   per genome g: connections conn_off[g]..conn_off[g+1]-1 in genome.connections order (in-key, out-key, weight, enabled);
 *   nodes node_off[g]..node_off[g+1]-1 (key, activation id or 255 if unknown, 1 if aggregation == "sum", bias, response).
 *   input_keys / output_keys: config.genome_config; leaves are numbered in input_keys order.
 * Outputs (caller-allocated, capacities cap_nodes / cap_edges): o_node_off [G+1], o_edge_off [nodes+1], o_act, o_bias,
 * o_resp, o_edge_src, o_edge_w, o_out_node [G][n_outputs].  o_status[g]: 0 done; 1 = a node whose inputs are ALL constants
 * would have to be folded with numpy's float32 activations -- the caller flattens that genome itself (its segment is
 * empty); 2 = the genome is invalid (cycle, unknown activation, unsupported aggregation, missing node): the caller's own
 * code raises the matching exception.  Returns EIGEN_OK, or EIGEN_ERR_CAPACITY if an output array is too small. */
int eigen_flatten_genomes(int32_t n_genomes, int32_t n_inputs, const int32_t* input_keys, int32_t n_outputs,
                          const int32_t* output_keys, const int32_t* conn_off, const int32_t* conn_in,
                          const int32_t* conn_out, const double* conn_w, const uint8_t* conn_enabled,
                          const int32_t* node_off, const int32_t* node_key, const uint8_t* node_act,
                          const uint8_t* node_agg_sum, const double* node_bias, const double* node_resp,
                          int32_t cap_nodes, int32_t cap_edges, int32_t* o_node_off, int32_t* o_edge_off, uint8_t* o_act,
                          double* o_bias, double* o_resp, int32_t* o_edge_src, double* o_edge_w, int32_t* o_out_node,
                          uint8_t* o_status);

/* Element-wise order of the ConvLSTM gate epilogue this library was compiled with (csrc/conv_mfma.h: EIG_GATE_ORDER):
 * 1 = chainer_prednet's ConvLSTM.__call__ where it is knowable (rounded peephole products, sigmoid = tanh(x/2)/2 + 1/2, un-fused
 * cell update), 0 = rounds 1-3.  The CPU oracle (oracle/eig_oracle.c: eig_oracle_gate_order) must report the same value. */
int eigen_gate_order(void);

/* Host-only, like eigen_flatten_genomes (no engine, no device): the launches of ONE PredNet step -- step0 != 0: the first step after reset_state(), otherwise a
 * steady-state step that is not the roll-out's last -- as csrc/conv_plan.h plans them for `batch` images on a device of n_cu compute units, with every EIGEN_* A/B
 * switch at its default (the environment is not read).  wino_mask: as eigen_winograd_mask reports it; < 0: the built-in default.  One text line per launch, in
 * launch order: "<convA|up4|lstm|convP> layer=.. kernel=<mfma|mfma_onekb|mfma_w8|convp0|lstm0|wino> shape=<tw16|tw8|pixel|wide|tall|half|pack> epi=.. wino=..
 * fused=.. vec=.. NI=.. n_nblk=.. tilesX=.. tilesY=.. nparts=.. nwalk=.. grid=.. threads=..".  Returns the length of the text (it was truncated to cap - 1
 * characters if that is >= cap) or a negative eigen_status. */
int eigen_plan_text(int32_t n_layers, const int32_t* channels, int32_t width, int32_t height, int32_t batch, int32_t n_cu,
                    int32_t wino_mask, int32_t step0, char* out, int32_t cap);

/* eigen_plan_text under given Winograd shape switches (same text, same return value): w4 = {EIGEN_W4_TALL, EIGEN_W4_HALF, EIGEN_W4_PACK, EIGEN_W4_PARTS} as
 * csrc/conv_plan.h reads them (-1, -1, -1, 0: the defaults, eigen_plan_text's plan), every other switch at its default.  w4 == NULL: what THIS process will launch --
 * every switch as the process read it from its environment, and wino_mask < 0 the mask eigen_winograd_mask reports. */
int eigen_plan_text_sw(int32_t n_layers, const int32_t* channels, int32_t width, int32_t height, int32_t batch, int32_t n_cu,
                       int32_t wino_mask, int32_t step0, const int32_t* w4, char* out, int32_t cap);

/* The EFFECTIVE operator-form mask of this process (csrc/eigen_engine.hip: EIGEN_WINOGRAD with EIGEN_WINO_FUSEUP=0 folded in as a cleared bit 24): which 3x3
 * convolutions run in which canonical summation order.  Every rank of a multi-GPU run must report the same value -- a population scored
 * under two orders still looks valid (bench.py gathers it).  The CPU oracle's oracle.wino_mask_default() states the same rule. */
int eigen_winograd_mask(void);

/* Deterministic fp32 exp / sigmoid / tanh used by the gate epilogue. */
int eigen_test_det_math(eigen_engine* e, const float* d_x, int32_t n, float* d_exp, float* d_sig, float* d_tanh,
                        void* stream);

/* Per-stage timing of the last eigen_eval_* call, milliseconds, measured with HIP events on the stream:
 * [0] render  [1] PredNet roll-out  [2] flow  [3] score  [4] PredNet conv kernels only (sum)
 * [5] number of conv kernel launches in the roll-out.
 * A dense call reports its stage as [2] and 0 as [3]; under EIGEN_DENSE_FLOAT_FRAMES the gray snapshots taken inside the roll-out fall
 * into [1], and the stage from the gray planes on (under EIGEN_PAIR_SINGLE with the gray of the input image) into [2]. */
int eigen_get_timings(eigen_engine* e, double* h_ms6);

/* Per-op profile of the roll-out convolutions.  enable=1 brackets every conv launch with HIP events recorded on the
 * launch stream (and waits for each).  h_out rows (8 doubles each, at most max_ops rows):
 * [layer, epilogue (1 LSTM, 2 ConvA, 3 ConvP, 4 packed LSTM, 5 / 6 the 2x2-form pass over the ConvLSTM's unpooled source (6: all four parity classes in one block); +32 for an operator in its Winograd F(4x4, 3x3) form (csrc/conv_wino4.h; FLOPs then count its 36 multiply-adds per channel and 4x4 outputs -- 25 for an unpooled source); +16 for the step-0 operators, which skip the sources
 *  that are identically zero after reset_state()), NI, TW, launches, total_ms, FLOPs per launch per image (2 x the
 *  multiply-accumulates executed), n_nblk].  At most 6 rows per layer.  reset=1 clears the accumulators after reading. */
int eigen_conv_profile(eigen_engine* e, int32_t enable, int32_t reset, double* h_out, int32_t max_ops, int32_t* n_ops);

/* Stage-level read-back for the parity tests: the dense field of the last eigen_flow call of an engine created with
 * flow_method = EIGEN_FLOW_FARNEBACK, float [batch][2][H][W] (dx plane, dy plane). */
int eigen_debug_dense_flow(eigen_engine* e, int32_t batch, float* h_flow, void* stream);

/* Stage-level read-back for the parity tests: one float32 tensor of the layer state that the last eigen_prednet_sequence call left
 * on the handle (its last step also runs ConvP_l for l > 0, so every tensor is of the same step).
 *   which = EIGEN_STATE_R: R_l (the ConvLSTM output h), EIGEN_STATE_C: the cell state c_l, EIGEN_STATE_P: the prediction P_l, each
 *   float [batch][C_l][H_l][W_l]; EIGEN_STATE_E: the error units E_l, float [batch][2 C_l][H_l][W_l] (relu(A - P), then relu(P - A)).
 *   E_l for l >= 1 belongs to the last executed step.  E_0 is the tensor that step CONSUMED -- err(its input frame, P_0 of the step
 *   before): the last step of a call does not write the next one, whose frame it has not seen (the next call forms it from the kept
 *   P_0 and its first input).  The CPU oracle's prednet_step leaves exactly that in E[0] (error_unit(x, P[0]) on entry).
 * Synchronises the stream and copies; no kernel is launched and the state is not changed.
 * Errors: EIGEN_ERR_STATE where a reset = 0 call of this batch would be refused (no call yet, a roll-out or evaluation since, another
 * batch); EIGEN_ERR_INVALID for a layer outside 0 .. n_layers - 1, an unknown `which` or a NULL pointer. */
enum eigen_state_tensor { EIGEN_STATE_R = 0, EIGEN_STATE_C = 1, EIGEN_STATE_P = 2, EIGEN_STATE_E = 3 };
int eigen_debug_state(eigen_engine* e, int32_t batch, int32_t layer, int32_t which, float* h_out, void* stream);

/* Stage-level read-back for the parity tests: corners / tracked points / status of the last eigen_flow call. */
int eigen_debug_corners(eigen_engine* e, int32_t batch, float* h_corners, int32_t* h_ncorners, float* h_next,
                        uint8_t* h_status, void* stream);

/* Algorithmic FLOPs (2 x MACs of the 3x3 convolutions) of one PredNet step for one genome. */
double eigen_prednet_flops_per_step(const eigen_engine* e);


/* ---------------------------------------------------------------------------------------------------- training
 * PredNet training on frame sequences: next-frame MSE or, per call, the error-unit objective L_0 / L_all
 * (eigen_trainer_loss_grad_obj), full backprop through time within a call, Adam as chainer defines it.  A separate handle: no inference handle's state or workspaces are touched.  Gradients and
 * weights are bit-identical from run to run (fixed-order reductions, no float atomics). */
typedef struct eigen_trainer eigen_trainer;

typedef struct {
    int32_t device;                        /* HIP device ordinal */
    int32_t width, height;                 /* both divisible by 2^(n_layers-1) */
    int32_t n_layers;
    int32_t channels[EIGEN_MAX_LAYERS];    /* channels[0] = 1 or 3 */
    int32_t max_batch;                     /* sequences per call (tape sizing) */
    int32_t max_steps;                     /* frames per call (tape sizing) */
} eigen_trainer_config;

int eigen_trainer_create(const eigen_trainer_config* cfg, eigen_trainer** out);
int eigen_trainer_destroy(eigen_trainer* t);

/* Host float32 tables in the order of eigen_set_prednet_weights.  set_weights also clears the Adam moments and step count
 * and discards any kept sequence state. */
int eigen_trainer_set_weights(eigen_trainer* t, const float* const* h_tensors, int32_t n_tensors);
int eigen_trainer_get_weights(eigen_trainer* t, float* const* h_tensors, int32_t n_tensors);

/* The training objective of one call (a per-call argument: the handle keeps nothing of it).
 *   EIGEN_OBJ_MSE: the squared error of the image-layer prediction against the next frame.
 *   EIGEN_OBJ_ERROR: PredNet's own objective (Lotter et al.), the mean of the error units, weighted per layer.
 *   EIGEN_OBJ_FLOW: the displacement a dense Lucas-Kanade solve finds from the next frame to the prediction; it needs settings,
 *     which only eigen_trainer_loss_grad_flow takes: every other entry refuses it. */
typedef enum { EIGEN_OBJ_MSE = 0, EIGEN_OBJ_ERROR = 1, EIGEN_OBJ_FLOW = 2 } eigen_objective;

/* Forward with a tape, loss and backward over one batch of sequences; OVERWRITES the gradients.
 *   d_frames: uint8 frames, frame s of sequence b at d_frames + b * bstride + s * C*H*W (bytes); n_steps frames each.
 *   reset = 1: start from zero state (needs n_steps >= 2).  reset = 0: start from the state (h, c, P) the previous call left,
 *     which must have had the same batch; that state is a constant (no gradient flows into the previous call).
 *   n_fed: steps s < n_fed read frame s (teacher-forced); steps s >= n_fed are self-fed: their input is the prediction
 *     P0_{s-1} (for s = 0: the kept P0).  0 <= n_fed <= n_steps; n_fed = 0 needs reset = 0.  All n_steps frames are still
 *     passed: on self-fed steps they are targets only.
 *   requant: how a prediction is fed back, as eigen_config.requant_feedback: 0 the float P0_{s-1} (E_0 is exactly zero);
 *     1 the byte the inference engine emits for it over 255, (float)(uint8_t)(int)(v * 255.0f) / 255.0f, a constant of the
 *     graph: E_0 = [relu(q - P0), relu(P0 - q)] is small, non-zero and sends a gradient into P0_{s-1} (relu'(0) = 0).
 *   h_step_w: host double[n_steps - 1], >= 0, finite, not all zero, or NULL (all ones): the weight w_s of term s.  A call owns
 *     its n_steps - 1 terms; term s belongs to step s + 1: the prediction P0_s after frame s against frame s + 1.  The term of
 *     the last prediction against the next call's first frame is in no call.
 *   objective = EIGEN_OBJ_MSE: with mse_s the mean over b, c, y, x of (P0_s - x_{s+1})^2, loss = sum_s w_s mse_s / sum_s w_s.
 *     With h_step_w = NULL it is one sum over all terms times 1 / ((n_steps-1) numel), formed on the device; with weights the mse_s
 *     are the numbers eigen_trainer_evaluate returns and the sum is done in double on the host, in step order.
 *   objective = EIGEN_OBJ_ERROR: loss = sum_s w_s sum_l lambda_l err[s][l] / sum_s w_s, formed on the host in double in (step,
 *     layer) order; lambda = h_layer_w.  The gradients are those of this loss (relu'(0) = 0, sign(0) = 0).
 *   err[s][l], s in [0, n_steps-2]:
 *     l = 0: the mean over b, the 2 C_0 error channels, y, x of [relu(x_{s+1} - P0_s), relu(P0_s - x_{s+1})], always against the
 *       TRUE frame x_{s+1} = (float)byte / 255.0f, on self-fed steps as well; it equals mean |P0_s - x_{s+1}| / 2.
 *     l > 0: the mean over b, 2 C_l, y, x of E_l of step s + 1, the errors the network itself computed there.
 *     The errors of the call's first step (the kept P against the first frame) belong to no call.
 *   h_layer_w: host double[n_layers], >= 0, finite, not all zero, or NULL: L_0, [1, 0, ...] (Lotter's L_all is [1, 0.1, ...]).
 *     Checked whenever it is given; used by EIGEN_OBJ_ERROR only.
 *   h_loss (host, may be NULL) receives the loss; d_pred (may be NULL) float [batch][n_steps][C][H][W] receives P0_s.
 *   h_layer_err (host, may be NULL): double[(n_steps-1) * n_layers], err[s][l] at s * n_layers + l, under either objective.
 *     Every entry is reduced in double over fixed slices in a fixed order: the same frames give the same bits from
 *     eigen_trainer_evaluate_err.
 * Errors: EIGEN_ERR_CAPACITY batch / n_steps above the handle's; EIGEN_ERR_STATE no weights, or reset = 0 without a previous
 * call of the same batch; EIGEN_ERR_INVALID n_steps < 2 with reset = 1, n_fed outside [0, n_steps], n_fed = 0 with reset = 1,
 * requant not 0 or 1, an unknown objective, a negative / non-finite step or layer weight, or weights that are all zero. */
int eigen_trainer_loss_grad_obj(eigen_trainer* t, const uint8_t* d_frames, int64_t bstride, int32_t batch, int32_t n_steps,
                                int32_t n_fed, int32_t requant, int32_t reset, const double* h_step_w, int32_t objective,
                                const double* h_layer_w, double* h_loss, double* h_layer_err, float* d_pred, void* stream);

/* eigen_trainer_loss_grad_obj plus d loss / d frames ("Frame gradients").  d_frame_grad NULL: exactly
 * eigen_trainer_loss_grad_obj, which is this call with NULL, 0, 0: the same launches, the same bits.
 *   d_frame_grad: device float; g_t = d loss / d x_t of sample b, step t at d_frame_grad + b * g_bstride + t * g_tstride as [C][H][W],
 *     strides in floats, x_t = (float)byte / 255.0f.  g_t is the sum of the input path (steps t < n_fed: dA of the image layer's
 *     error unit, relu'(0) = 0) and the target path (t >= 1: frame t is the target of term t - 1 under either objective, on
 *     self-fed steps too; sign(0) = 0; a term whose weight is zero adds nothing).  Frame 0 of a call has no target path.
 *   g_tstride == 0: tied, for a still repeated n_steps times: one image per sample, cleared by the call, then g_t added in
 *     float in the order t = n_steps - 1 .. 0.  Otherwise g_tstride >= C*H*W.  g_bstride >= the extent of one sample (C*H*W tied,
 *     (n_steps - 1) * g_tstride + C*H*W otherwise).  Floats between the images are never written.
 * Everything else the call returns (loss, table, predictions, weight gradients, kept state) is what it returns without d_frame_grad.
 * Errors: as eigen_trainer_loss_grad_obj; EIGEN_ERR_INVALID for a g_tstride in [1, C*H*W - 1] or < 0, or too small a g_bstride. */
int eigen_trainer_loss_grad_frames(eigen_trainer* t, const uint8_t* d_frames, int64_t bstride, int32_t batch, int32_t n_steps,
                                   int32_t n_fed, int32_t requant, int32_t reset, const double* h_step_w, int32_t objective,
                                   const double* h_layer_w, double* h_loss, double* h_layer_err, float* d_pred, float* d_frame_grad,
                                   int64_t g_bstride, int64_t g_tstride, void* stream);

/* Settings of EIGEN_OBJ_FLOW ("The flow objective"): the window is the pixels within Chebyshev radius
 * `radius` (1 .. 16) that lie inside the image; eps (finite, > 0) is added to the diagonal of the 2x2 system, in units of summed
 * squared gradients of images in [0, 1].
 * flags, bit 0, EIGEN_FLOW_MOVING_REFERENCE (eigen_trainer_loss_grad_flow only): the reference frame of every term is part of the
 * graph, not a constant of it.  Default (0): every call launches what it launched before the flag existed. */
#define EIGEN_FLOW_MOVING_REFERENCE 1
typedef struct {
    int32_t radius;
    int32_t flags;      /* 0, or EIGEN_FLOW_MOVING_REFERENCE where an entry takes it; any other bit is refused */
    double eps;
} eigen_flow_settings;

/* The flow stage alone, on one prediction / reference pair per sample; it runs the kernels a training call runs.  All arithmetic is
 * float64 on the device, one IEEE operation per operation written:
 *   gray: C = 1: I = v; C = 3: I = (0.299 v0 + 0.587 v1) + 0.114 v2; I0 from the reference ((float)byte / 255.0f), I1 from the
 *     prediction, It = I1 - I0.  Ix, Iy: the normalised Scharr derivative of I0 alone, indices clamped to the image.
 *   window sums Gxx, Gxy, Gyy, bx, by of Ix Ix, Ix Iy, Iy Iy, Ix It, Iy It over the truncated window: rows first, then columns,
 *     offsets ascending, each sum started from its first term.
 *   a = Gxx + eps, c = Gyy + eps, b = Gxy, det = a c - b b, ux = -((c bx - b by) / det), uy = -((a by - b bx) / det), pixels per frame.
 *   v = ux ux + uy uy, or dx ux + dy uy with a direction field; value = sum_b sum_p m(p) v / (batch N_m), N_m the count of the mask,
 *     reduced in double over fixed slices in a fixed order.
 *   seed = scale * d value / d prediction, exact because I0 is a constant: g = (2 ux, 2 uy) or d, q = m ((c gx - b gy) / det,
 *     (a gy - b gx) / det), Q = the window sums of q, t = Ix Qx + Iy Qy, s = -(t kappa), kappa = scale / (batch N_m) formed in double on
 *     the host, seed[c] = (float)(k_c s), k = (0.299, 0.587, 0.114) or (1).
 *   d_pred: float, sample b at d_pred + b * p_bstride (floats) as [C][H][W]; d_ref: uint8, sample b at d_ref + b * r_bstride (bytes).
 *   d_dir: float [2][H][W] (x then y component), shared by the batch, or NULL: the energy mode.  d_mask: uint8 [H][W], 0 = not counted,
 *     or NULL: all ones.
 *   Outputs, each may be NULL: h_value (host double); d_flow double [batch][2][H][W]; d_seed float, sample b at d_seed + b * s_bstride
 *     (floats) as [C][H][W]; floats between the samples are never written.
 * It needs no weights and touches neither gradients nor the kept state.
 * Errors: EIGEN_ERR_INVALID a NULL handle, prediction, reference or settings, batch < 1, a stride below C*H*W, radius outside 1 .. 16,
 * eps not finite or <= 0, non-zero flags, scale not finite, a direction that is not finite, a mask without a non-zero pixel;
 * EIGEN_ERR_CAPACITY batch above max_batch.  A refused call launches and writes nothing. */
int eigen_trainer_flow_term(eigen_trainer* t, const float* d_pred, int64_t p_bstride, const uint8_t* d_ref, int64_t r_bstride,
                            int32_t batch, const eigen_flow_settings* flow, const float* d_dir, const uint8_t* d_mask, double scale,
                            double* h_value, double* d_flow, float* d_seed, int64_t s_bstride, void* stream);

/* eigen_trainer_loss_grad_frames plus the flow objective.  objective = EIGEN_OBJ_FLOW: term s is the value of
 * eigen_trainer_flow_term for the prediction P0_s against frame s + 1 (the pairing of the other objectives), loss = sum_s w_s f_s /
 * sum_s w_s formed on the host in double in step order; a term with w_s = 0 is not computed and reports 0.0.  Its seed, with scale =
 * w_s / sum w, is added in float to d loss / d P0_s ahead of the clamp's mask, where the squared-error seed enters under
 * EIGEN_OBJ_MSE.  By default the frames are constants of the flow term: d_frame_grad holds the input path alone.
 *   flow->flags & EIGEN_FLOW_MOVING_REFERENCE: frame s + 1, the reference of term s, is in the graph.  Every computed term (w_s != 0)
 *     then adds the gradient eigen_trainer_flow_term_ref states, with scale = w_s / sum w, in float to d_frame_grad: per frame
 *     (g_tstride != 0) g_t = fl(input path of step t + reference path of term t - 1); tied (g_tstride == 0) the image starts from zero
 *     and for s = n_steps - 1 .. 0 first the reference path of term s is added, then the input path of step s.  Self-fed steps have
 *     a reference path too: targets stay the true frames.  Without d_frame_grad the bit changes nothing, and loss, terms, weight
 *     gradients, predictions and the kept state are the same bits with it and without.  Any other bit: EIGEN_ERR_INVALID.
 *   flow: the settings, required under EIGEN_OBJ_FLOW; d_dir, d_mask as eigen_trainer_flow_term.  Under another objective flow, d_dir
 *     and d_mask must be NULL and the call is eigen_trainer_loss_grad_frames.
 *   h_terms (host, may be NULL): double[n_steps - 1], the terms f_s; written under EIGEN_OBJ_FLOW only.
 * Errors: as eigen_trainer_loss_grad_frames and eigen_trainer_flow_term. */
int eigen_trainer_loss_grad_flow(eigen_trainer* t, const uint8_t* d_frames, int64_t bstride, int32_t batch, int32_t n_steps,
                                 int32_t n_fed, int32_t requant, int32_t reset, const double* h_step_w, int32_t objective,
                                 const double* h_layer_w, double* h_loss, double* h_layer_err, float* d_pred, float* d_frame_grad,
                                 int64_t g_bstride, int64_t g_tstride, const eigen_flow_settings* flow, const float* d_dir,
                                 const uint8_t* d_mask, double* h_terms, void* stream);

/* eigen_trainer_flow_term plus the gradient of the term by its REFERENCE frame, scale * d value / d x with x = (float)byte / 255.0f
 * the reference's floats: the kernels a training call runs under EIGEN_FLOW_MOVING_REFERENCE.  Float64, one IEEE operation per
 * operation written.  With u, q, Q, Ix, Iy, It and kappa of eigen_trainer_flow_term:
 *   window sums (the same order) Mxx = sum 2 (qx ux), Mxy = sum (qx uy + qy ux), Myy = sum 2 (qy uy);
 *   rx = -(((Qx It + Mxx Ix) + Mxy Iy) kappa), ry = -(((Qy It + Mxy Ix) + Myy Iy) kappa), e = (Ix Qx + Iy Qy) kappa;
 *   d = e + S^T(rx, ry), S^T the adjoint of the normalised Scharr pair with clamped indices: a tap the forward pass clamps onto a
 *     border pixel sends its share back to that pixel (csrc/flow_ref_kernels.h fixes the order of the additions);
 *   d_ref_grad[c] = (float)(k_c d), k = (0.299, 0.587, 0.114) or (1): sample b at d_ref_grad + b * rg_bstride (floats) as [C][H][W],
 *     a plain store; floats between the samples are never written.
 * Errors: as eigen_trainer_flow_term (non-zero flags among them: the entry is the request); EIGEN_ERR_INVALID a NULL d_ref_grad or an
 * rg_bstride below C*H*W. */
int eigen_trainer_flow_term_ref(eigen_trainer* t, const float* d_pred, int64_t p_bstride, const uint8_t* d_ref, int64_t r_bstride,
                                int32_t batch, const eigen_flow_settings* flow, const float* d_dir, const uint8_t* d_mask, double scale,
                                double* h_value, double* d_flow, float* d_seed, int64_t s_bstride, float* d_ref_grad, int64_t rg_bstride,
                                void* stream);

/* The pairing of EIGEN_OBJ_FLOW ("The prediction pairing"): which image is the reference of term s.
 *   EIGEN_FLOW_PAIR_FRAME: frame s + 1, bytes; eigen_trainer_loss_grad_flow.  For a repeated still that is "still -> extended
 *     prediction", the pairing of EIGEN_PAIR_SINGLE.
 *   EIGEN_FLOW_PAIR_PREDICTION: the previous prediction P0_{s-1}, floats, itself part of the graph; for s = 0 the start state's P of
 *     layer 0 (zeros after a reset, the kept P of a continued call), a constant of the call.  With step weights that select the term
 *     "prediction after the last fed frame -> first extended prediction" that is what EIGEN_PAIR_POPULATION scores. */
enum { EIGEN_FLOW_PAIR_FRAME = 0, EIGEN_FLOW_PAIR_PREDICTION = 1 };

/* eigen_trainer_loss_grad_flow plus the pairing.  EIGEN_FLOW_PAIR_FRAME: the call IS eigen_trainer_loss_grad_flow, launch for launch and
 * bit for bit.  EIGEN_FLOW_PAIR_PREDICTION (objective EIGEN_OBJ_FLOW only): term s is the value of eigen_trainer_flow_term_pair for P0_s
 * against P0_{s-1}; loss and h_terms are those of this pairing, a term with w_s = 0 is not computed and reports 0.0.  Every computed
 * term has two seeds, both with scale = w_s / sum w: its seed by P0_s, added in float to d loss / d P0_s ahead of the clamp's mask as
 * under the frame pairing, and, for s >= 1, its gradient by its reference (d_prev_grad of eigen_trainer_flow_term_pair), added in float
 * to d loss / d P0_{s-1} ahead of that step's clamp mask.  The float additions into d loss / d P0_{s-1} come in this order: what layer
 * 0's error units of step s leave there; then the reference path of term s; then the seed of term s - 1.  Self-fed steps need nothing
 * special: with requantised feedback the fed-back byte is a constant as before while the reference of the term stays the float
 * P0_{s-1}.  Frames are no references: d_frame_grad holds the input path alone, which is the whole gradient.
 * Errors: as eigen_trainer_loss_grad_flow; EIGEN_ERR_INVALID, before any launch, an unknown pairing, EIGEN_FLOW_PAIR_PREDICTION under
 * another objective, and EIGEN_FLOW_PAIR_PREDICTION together with EIGEN_FLOW_MOVING_REFERENCE. */
int eigen_trainer_loss_grad_flow_pair(eigen_trainer* t, const uint8_t* d_frames, int64_t bstride, int32_t batch, int32_t n_steps,
                                      int32_t n_fed, int32_t requant, int32_t reset, const double* h_step_w, int32_t objective,
                                      const double* h_layer_w, double* h_loss, double* h_layer_err, float* d_pred, float* d_frame_grad,
                                      int64_t g_bstride, int64_t g_tstride, const eigen_flow_settings* flow, const float* d_dir,
                                      const uint8_t* d_mask, double* h_terms, int32_t pairing, void* stream);

/* The flow stage alone on one pair of FLOAT images per sample, with the kernels a training call runs under
 * EIGEN_FLOW_PAIR_PREDICTION: eigen_trainer_flow_term with I0 the gray of d_prev (floats widened to double; sample b at d_prev + b *
 * r_bstride floats as [C][H][W]) in place of the reference bytes.  d_prev_grad (may be NULL): scale * d value / d d_prev, the gradient
 * eigen_trainer_flow_term_ref states, float, sample b at d_prev_grad + b * pg_bstride as [C][H][W], a plain store.  With d_prev =
 * (float)byte / 255.0f of a frame every output is eigen_trainer_flow_term_ref's on that frame, bit for bit.
 * Errors: as eigen_trainer_flow_term (non-zero flags among them); EIGEN_ERR_INVALID a NULL d_prev, or a pg_bstride below C*H*W when
 * d_prev_grad is given. */
int eigen_trainer_flow_term_pair(eigen_trainer* t, const float* d_pred, int64_t p_bstride, const float* d_prev, int64_t r_bstride,
                                 int32_t batch, const eigen_flow_settings* flow, const float* d_dir, const uint8_t* d_mask, double scale,
                                 double* h_value, double* d_flow, float* d_seed, int64_t s_bstride, float* d_prev_grad, int64_t pg_bstride,
                                 void* stream);

/* The score mode of EIGEN_OBJ_FLOW ("The score mode"; csrc/flow_score_kernels.h fixes every order): the value of
 * a term is the Circles score of the population fitness on the dense field u of eigen_trainer_flow_term's solve, which is unchanged.
 * Float64 on the device, one IEEE operation per operation written.  Per sample b and pixel (x, y):
 *   px = x - W / 2.0, py = y - H / 2.0, dist = sqrt(px px + py py), nrm = sqrt(ux ux + uy uy);
 *   member: the mask counts the pixel, dist != 0, r_min <= dist <= r_max, nrm > 0, min_norm <= nrm <= max_norm; membership is a constant
 *     of the graph;
 *   nx = ux / nrm, ny = uy / nrm, x1 = px + nx, y1 = py + ny, rho = (x1 px + y1 py) / dist - dist, tau = (-x1 py + y1 px) / dist;
 *   over the N members, two passes: the means m_rho, m_tau, m_a of |ux|, m_n of nrm; then V_rho, V_tau, V_n, the mean squared
 *     deviations from them; fixed slices, fixed order;
 *   R = ((1 - V_rho)(1 - V_rho) + (1 - V_tau)(1 - V_tau)) / 2, A = m_a / max_norm, F = 1 - min(V_n, 1),
 *     S_b = w_direction R + w_strength (A F), or 0 with N < min_count; value f = (sum_b S_b) / batch, b ascending.
 *   g = d S_b / d u at the members, 0 elsewhere and in a sample below min_count; q = ((c gx - b gy) / det, (a gy - b gx) / det), 0 where
 *     the pixel is no member; seed and reference gradient are eigen_trainer_flow_term's and eigen_trainer_flow_term_ref's from this q
 *     with kappa = scale / batch: the mask's count does not enter.
 * reserved must be 0. */
typedef struct {
    double max_norm, min_norm;   /* finite max_norm > 0; 0 <= min_norm < max_norm: the gradient carries 1 / nrm */
    double r_min, r_max;         /* finite, 0 <= r_min <= r_max: the ring of distances from (W / 2, H / 2) */
    double w_direction, w_strength; /* finite, >= 0, not both 0 */
    int32_t min_count, reserved; /* min_count >= 2: a sample with fewer members scores 0; reserved must be 0 */
} eigen_flow_score;

/* The flow stage alone in the score mode, with the kernels a training call runs.  Arguments as eigen_trainer_flow_term_ref /
 * eigen_trainer_flow_term_pair, with these differences: the reference is bytes (d_ref) or floats (d_fref), exactly one of them
 * non-NULL, sample b at + b * r_bstride; there is no direction field; score is required; h_stats (host, may be NULL) receives
 * double[batch][10]: N, m_rho, m_tau, m_a, m_n, V_rho, V_tau, V_n, S_b and a spare 0.  d_ref_grad (may be NULL) is stored as
 * eigen_trainer_flow_term_ref / _pair store theirs.
 * Errors: as eigen_trainer_flow_term; EIGEN_ERR_INVALID, before any launch: a NULL score, both or neither reference, max_norm not
 * finite or <= 0, min_norm outside [0, max_norm), r_min < 0, r_max < r_min or either not finite, min_count < 2, a weight that is
 * negative or not finite, both weights zero, reserved != 0. */
int eigen_trainer_flow_term_score(eigen_trainer* t, const float* d_pred, int64_t p_bstride, const uint8_t* d_ref, const float* d_fref,
                                  int64_t r_bstride, int32_t batch, const eigen_flow_settings* flow, const uint8_t* d_mask,
                                  const eigen_flow_score* score, double scale, double* h_value, double* h_stats, double* d_flow,
                                  float* d_seed, int64_t s_bstride, float* d_ref_grad, int64_t rg_bstride, void* stream);

/* eigen_trainer_loss_grad_flow_pair plus the score.  score == NULL: the call IS eigen_trainer_loss_grad_flow_pair, launch for launch and
 * bit for bit.  Otherwise (objective EIGEN_OBJ_FLOW only, d_dir NULL) every computed term is the value of eigen_trainer_flow_term_score
 * under the call's pairing, its seeds carry scale = w_s / sum w with kappa = scale / batch, and everything else, the moving reference
 * under the frame pairing included, is as without a score.
 * Errors: as eigen_trainer_loss_grad_flow_pair and eigen_trainer_flow_term_score; EIGEN_ERR_INVALID a score under another objective or
 * together with a direction field. */
int eigen_trainer_loss_grad_flow_score(eigen_trainer* t, const uint8_t* d_frames, int64_t bstride, int32_t batch, int32_t n_steps,
                                       int32_t n_fed, int32_t requant, int32_t reset, const double* h_step_w, int32_t objective,
                                       const double* h_layer_w, double* h_loss, double* h_layer_err, float* d_pred, float* d_frame_grad,
                                       int64_t g_bstride, int64_t g_tstride, const eigen_flow_settings* flow, const float* d_dir,
                                       const uint8_t* d_mask, double* h_terms, int32_t pairing, const eigen_flow_score* score, void* stream);

/* The structure scores of EIGEN_OBJ_FLOW ("The structure scores"; csrc/flow_struct_kernels.h fixes every order):
 * the value of a term is the population fitness's score of the Bands structure (0: horizontal_symmetry_score) or of the Free structure
 * (2: 0.5 swarm_score + 0.1 strength_number + 0.4 min(n, 15) / 15), on the dense field u of eigen_trainer_flow_term's solve, which is
 * unchanged.  Structures 1 and 3 (Circles, CirclesFree) are the score mode's, eigen_flow_score.  Float64 on the device.  Common:
 *   nrm = sqrt(ux ux + uy uy); member: the mask counts the pixel, the structure's rule holds, nrm > 0, min_norm <= nrm <= max_norm, a
 *   constant of the graph; nx = ux / nrm, ny = uy / nrm; a sample with N < min_count members has S_b = 0 and passes no gradient;
 *   value f = (sum_b S_b) / batch; kappa = scale / batch; q from g = d S_b / d u as in the score mode, 0 off the members.
 * Bands: rule lim_lo <= y <= lim_hi, middle = (int)(lim_hi / 2); y < middle: (mx, my) = (nx, nx), else (-nx, ny); two passes:
 *   m_x, m_y, then V = mean (mx - m_x)^2; S_b = ((1 - V) + |m_x| + (1 - |m_y|)) / 3.  max_distance and w are not read.
 * Free: no rule; theta = acos(nx); over ordered pairs of members (i, j), i = j included: f = min(d2 / (max_distance max_distance), 1),
 *   close iff f < 1, opt = fmod(theta_i + f pi, 2) pi, L_i = sum_j close |theta_j - opt|, swarm = mean_i (pi - L_i / N) / pi;
 *   A = mean |ux| / max_norm, F = 1 - min(var nrm, 1); S_b = (w[0] swarm + w[1] (A F)) + w[2] (min(N, 15) / 15).  The limits are not read.
 * The record of a sample, double[10]: Bands N, m_x, m_y, V, 0, 0, 0, 0, S_b, 0; Free N, m_a, m_n, V_n, swarm, A F, 0, 0, S_b, 0. */
typedef struct {
    int32_t structure, min_count; /* 0 Bands, 2 Free; min_count >= 1: a sample with fewer members scores 0 */
    double max_norm, min_norm, lim_lo, lim_hi, max_distance, w[3];
} eigen_flow_structure_score;

/* The flow stage alone under a structure score: eigen_trainer_flow_term_score's arguments with the structure score in place of the
 * score; h_stats (host, may be NULL) receives double[batch][10], the records above.
 * Errors: as eigen_trainer_flow_term_score; EIGEN_ERR_INVALID, before any launch: a NULL score, structure 1 or 3 (the message names
 * eigen_flow_score) or unknown, max_norm not finite or <= 0, min_norm outside [0, max_norm), min_count < 1; Bands: limits not finite,
 * lim_hi < lim_lo or |lim_hi| > 2e9 (middle is an int); Free: max_distance not finite or <= 0, a weight that is negative or not finite, all weights zero. */
int eigen_trainer_flow_term_structure(eigen_trainer* t, const float* d_pred, int64_t p_bstride, const uint8_t* d_ref, const float* d_fref,
                                      int64_t r_bstride, int32_t batch, const eigen_flow_settings* flow, const uint8_t* d_mask,
                                      const eigen_flow_structure_score* score, double scale, double* h_value, double* h_stats, double* d_flow,
                                      float* d_seed, int64_t s_bstride, float* d_ref_grad, int64_t rg_bstride, void* stream);

/* Debug: what the last Free stage of this handle (eigen_trainer_flow_term_structure, or the last computed term of a training call) left in
 * the workspace of its pair pass, copied to the host; every target may be NULL, each is [batch][H][W]: theta = acos(nx) and the member
 * flag of every pixel (0 off the members), L_i, and the integer sign sums rowS_i and colS_i.  No kernel is launched.  Before any Free
 * stage the planes hold nothing defined.  Errors: EIGEN_ERR_INVALID a NULL handle or a batch outside 1 .. max_batch. */
int eigen_trainer_debug_free_planes(eigen_trainer* t, int32_t batch, double* h_theta, double* h_L, int32_t* h_rowS, int32_t* h_colS,
                                    uint8_t* h_flag, void* stream);

/* eigen_trainer_loss_grad_flow_pair plus the structure score.  score == NULL: the call IS eigen_trainer_loss_grad_flow_pair, launch for
 * launch and bit for bit.  Otherwise (objective EIGEN_OBJ_FLOW only, d_dir NULL) every computed term is the value of
 * eigen_trainer_flow_term_structure under the call's pairing, with kappa = (w_s / sum w) / batch; the moving reference under the frame
 * pairing works as without a score.
 * Errors: as eigen_trainer_loss_grad_flow_pair and eigen_trainer_flow_term_structure; EIGEN_ERR_INVALID a structure score under another
 * objective or together with a direction field. */
int eigen_trainer_loss_grad_flow_structure(eigen_trainer* t, const uint8_t* d_frames, int64_t bstride, int32_t batch, int32_t n_steps,
                                           int32_t n_fed, int32_t requant, int32_t reset, const double* h_step_w, int32_t objective,
                                           const double* h_layer_w, double* h_loss, double* h_layer_err, float* d_pred, float* d_frame_grad,
                                           int64_t g_bstride, int64_t g_tstride, const eigen_flow_settings* flow, const float* d_dir,
                                           const uint8_t* d_mask, double* h_terms, int32_t pairing, const eigen_flow_structure_score* score,
                                           void* stream);

/* Per-sample membership of the scores of EIGEN_OBJ_FLOW ("The corner members"; csrc/flow_corner_kernels.h).  A score's
 * member rule reads "the mask counts the pixel"; with members that mask is one plane per sample: the mask byte of sample b, pixel p is
 * mask[b * mask_bstride + p].  The score's geometric rule and its norm limits apply on top, and membership stays a constant of the graph.
 *   EIGEN_FLOW_MEMBERS_MASK: d_mask holds the planes, mask_bstride >= H*W bytes apart.  A plane set that counts no pixel at all is
 *     refused; a single sample that counts none scores 0.
 *   EIGEN_FLOW_MEMBERS_CORNERS: the members of a term are the corners the fitness would pick on the term's own reference, derived on the
 *     device in front of the term's stage: the reference as bytes (a byte reference as it is; a float one clamped to [0, 1], then
 *     (uint8_t)(int)(v * 255.0f), the byte a self-fed step reads), then cvtColor / cornerMinEigenVal(block_size, 3) /
 *     goodFeaturesToTrack(max_corners, quality_level, min_distance) with eigen_flow's own kernels.  d_mask, if given, is the shared
 *     [H][W] plane: a corner it does not count is no member.  The workspace is allocated by the first call that needs it and freed with the
 *     handle; eigen_trainer_tape_bytes does not count it. */
enum { EIGEN_FLOW_MEMBERS_MASK = 0, EIGEN_FLOW_MEMBERS_CORNERS = 1 };
typedef struct {
    int32_t kind;            /* MASK: d_mask holds one plane per sample; CORNERS: derived from each term's reference */
    int32_t max_corners;     /* CORNERS: 1 .. 128 */
    int32_t block_size, reserved; /* block_size, CORNERS: 1 .. 9, what mineig_kernel's staged tile holds; reserved: 0 */
    double quality_level;    /* CORNERS: in (0, 1] */
    double min_distance;     /* CORNERS: finite, >= 0 */
    int64_t mask_bstride;    /* MASK: >= H*W; CORNERS: 0 (d_mask, if given, is the shared [H][W] plane) */
} eigen_flow_members;

/* The membership stage alone (kind EIGEN_FLOW_MEMBERS_CORNERS): the corners of batch references, bytes (d_ref) or floats (d_fref), exactly
 * one of the two non-NULL, sample b at + b * r_bstride elements.  h_members (host, may be NULL) receives uint8 [batch][H][W], 1 at every
 * corner the shared plane d_mask (may be NULL) counts; h_counts (host, may be NULL) int32 [batch], the corners selected per sample, before
 * the mask.  The call synchronises the stream.
 * Errors: EIGEN_ERR_INVALID, before any launch: a NULL handle or members, both or neither reference, batch < 1, r_bstride < C*H*W, a kind
 * other than CORNERS, reserved != 0, max_corners outside 1 .. 128, block_size outside 1 .. 9, quality_level outside (0, 1], min_distance
 * negative or not finite, mask_bstride != 0; EIGEN_ERR_CAPACITY batch above max_batch. */
int eigen_trainer_flow_members(eigen_trainer* t, const uint8_t* d_ref, const float* d_fref, int64_t r_bstride, int32_t batch,
                               const eigen_flow_members* members, const uint8_t* d_mask, uint8_t* h_members, int32_t* h_counts, void* stream);

/* The flow stage alone, the widest entry: eigen_trainer_flow_term_score's arguments with exactly one of score and sscore non-NULL, plus
 * members (NULL: the call IS eigen_trainer_flow_term_score / eigen_trainer_flow_term_structure, launch for launch and bit for bit).
 * Under CORNERS the membership stage runs on the call's reference in front of the stage.
 * Errors: as those two entries; EIGEN_ERR_INVALID, before any launch: members without a score (the displacement modes divide by a
 * host-side mask count), both scores, an unknown kind, reserved != 0, a field outside the range the struct states, MASK with
 * mask_bstride < H*W or without d_mask or with planes that count no pixel at all; the message names the field. */
int eigen_trainer_flow_term_members(eigen_trainer* t, const float* d_pred, int64_t p_bstride, const uint8_t* d_ref, const float* d_fref,
                                    int64_t r_bstride, int32_t batch, const eigen_flow_settings* flow, const uint8_t* d_mask,
                                    const eigen_flow_score* score, const eigen_flow_structure_score* sscore, const eigen_flow_members* members,
                                    double scale, double* h_value, double* h_stats, double* d_flow, float* d_seed, int64_t s_bstride,
                                    float* d_ref_grad, int64_t rg_bstride, void* stream);

/* The widest training entry: eigen_trainer_loss_grad_flow_score and eigen_trainer_loss_grad_flow_structure in one (at most one of score
 * and sscore non-NULL) plus members and h_stats.  members == NULL and h_stats == NULL: the call IS the entry of its score, launch for
 * launch and bit for bit.  Under CORNERS every term of non-zero weight runs the membership stage on its own reference in front of its
 * stage: frame s + 1 under the frame pairing, P0_{s-1} under the prediction pairing (for s = 0 the start state's P: after a reset it is
 * zero, there are no corners, and the term is 0 with no gradient).  h_stats (host, may be NULL; read with a score only) receives
 * double[n_steps - 1][batch][10], the samples' records of every computed term and zeros for the others.
 * Errors: as those entries and eigen_trainer_flow_term_members; EIGEN_ERR_INVALID members under another objective. */
int eigen_trainer_loss_grad_flow_members(eigen_trainer* t, const uint8_t* d_frames, int64_t bstride, int32_t batch, int32_t n_steps,
                                         int32_t n_fed, int32_t requant, int32_t reset, const double* h_step_w, int32_t objective,
                                         const double* h_layer_w, double* h_loss, double* h_layer_err, float* d_pred, float* d_frame_grad,
                                         int64_t g_bstride, int64_t g_tstride, const eigen_flow_settings* flow, const float* d_dir,
                                         const uint8_t* d_mask, double* h_terms, int32_t pairing, const eigen_flow_score* score,
                                         const eigen_flow_structure_score* sscore, const eigen_flow_members* members, double* h_stats,
                                         void* stream);

/* One normalised ascent step on uint8 stills d_images [batch][C][H][W], in place, from a tied gradient (image b at d_grad + b *
 * g_bstride floats): per image m_b = max |g| over the pixels the mask keeps free, then x = byte / 255.0f,
 * x' = min(max(x + k * (g / m_b), 0), 1) with k = (float)(step_bytes / 255.0), byte' = (uint8_t)(int)(x' * 255.0f + 0.5f), each one
 * float operation.  d_mask: uint8 [H][W] shared by the channels, 0 = keep the pixel's byte, or NULL: every pixel moves.  An image
 * with m_b == 0 is left as it is.  No byte moves by more than ceil(step_bytes).
 * Errors: EIGEN_ERR_INVALID a NULL image or gradient, step_bytes not finite or <= 0, batch < 1, g_bstride < C*H*W;
 * EIGEN_ERR_CAPACITY batch above max_batch. */
int eigen_trainer_still_step(eigen_trainer* t, uint8_t* d_images, const float* d_grad, int64_t g_bstride, const uint8_t* d_mask,
                             double step_bytes, int32_t batch, void* stream);

/* eigen_trainer_loss_grad_obj with objective = EIGEN_OBJ_MSE, h_layer_w = NULL, h_layer_err = NULL. */
int eigen_trainer_loss_grad_ext(eigen_trainer* t, const uint8_t* d_frames, int64_t bstride, int32_t batch, int32_t n_steps,
                                int32_t n_fed, int32_t requant, int32_t reset, const double* h_step_w, double* h_loss,
                                float* d_pred, void* stream);

/* eigen_trainer_loss_grad_ext with n_fed = n_steps, requant = 0, h_step_w = NULL. */
int eigen_trainer_loss_grad(eigen_trainer* t, const uint8_t* d_frames, int64_t bstride, int32_t batch, int32_t n_steps,
                            int32_t reset, double* h_loss, float* d_pred, void* stream);

/* Forward only, without a tape: the per-step losses of a sequence of ANY length (n_steps is not bounded by max_steps; batch <=
 * max_batch).  d_frames, bstride, batch, n_fed, requant and reset as eigen_trainer_loss_grad_obj.  Touches neither the gradients
 * (a following eigen_trainer_adam still applies those of the last loss_grad) nor the Adam state.  It shares the kept sequence
 * state (h, c, P) with loss_grad: there is one state per handle, every call of either leaves its final state, and a reset = 0
 * call of either continues it.
 *   h_step_loss (host, may be NULL): double[n_steps - 1], the unweighted mse_s of every step.
 *   h_layer_err (host, may be NULL): double[(n_steps-1) * n_layers], the table err[s][l] of eigen_trainer_loss_grad_obj.
 *   d_pred (may be NULL): float [batch][n_steps][C][H][W].
 * Errors: as eigen_trainer_loss_grad_obj, without the bound on n_steps. */
int eigen_trainer_evaluate_err(eigen_trainer* t, const uint8_t* d_frames, int64_t bstride, int32_t batch, int32_t n_steps,
                               int32_t n_fed, int32_t requant, int32_t reset, double* h_step_loss, double* h_layer_err,
                               float* d_pred, void* stream);

/* eigen_trainer_evaluate_err with h_layer_err = NULL. */
int eigen_trainer_evaluate(eigen_trainer* t, const uint8_t* d_frames, int64_t bstride, int32_t batch, int32_t n_steps,
                           int32_t n_fed, int32_t requant, int32_t reset, double* h_step_loss, float* d_pred, void* stream);

/* Everything a continued run depends on besides the weights.
 *   h_m, h_v: the Adam first and second moments, host tables in eigen_set_prednet_weights order (get: both or neither).
 *   adam_t: the step count.  seq_batch: the batch of the kept sequence state, 0 when there is none.
 *   h_seq: 3 * n_layers host arrays, (h, c, P) of layer 0, then of layer 1, ...: each float [seq_batch][C_l][H_l][W_l].
 * get_state: every output may be NULL; h_seq is written only when *seq_batch > 0 (call once with h_seq = NULL to size it).
 * set_state: called after eigen_trainer_set_weights (which clears all of this).  seq_batch = 0 discards the sequence state
 *   (h_seq may be NULL); otherwise the next reset = 0 call of that batch continues from h_seq.
 * Errors: EIGEN_ERR_STATE no weights; EIGEN_ERR_INVALID a wrong n_tensors / n_seq, a NULL array, adam_t or seq_batch < 0;
 * EIGEN_ERR_CAPACITY seq_batch above max_batch. */
int eigen_trainer_get_state(eigen_trainer* t, float* const* h_m, float* const* h_v, int32_t n_tensors, int32_t* adam_t,
                            int32_t* seq_batch, float* const* h_seq, int32_t n_seq);
int eigen_trainer_set_state(eigen_trainer* t, const float* const* h_m, const float* const* h_v, int32_t n_tensors,
                            int32_t adam_t, int32_t seq_batch, const float* const* h_seq, int32_t n_seq);

/* The gradients of the last eigen_trainer_loss_grad / _ext / _obj, host tables in eigen_set_prednet_weights order. */
int eigen_trainer_get_grads(eigen_trainer* t, float* const* h_tensors, int32_t n_tensors);

/* One Adam step on the current gradients (step count kept by the handle, from 1): m += (1-beta1)(g-m),
 * v += (1-beta2)(g^2-v), p -= lr_t m / (sqrt(v) + eps), lr_t = alpha sqrt(1-beta2^t) / (1-beta1^t). */
int eigen_trainer_adam(eigen_trainer* t, double alpha, double beta1, double beta2, double eps, void* stream);

/* ---- Optimiser controls ("Optimiser controls"): what a training loop puts between the gradient and the
 * update.  All of it runs on the device, on the handle's float32 tables, with float64 reductions of a fixed partition and a fixed
 * order (no atomics): norms, clipped steps and accumulated gradients are the same bits from run to run. */

/* The settings of one eigen_trainer_adam_ex step.  alpha, beta1, beta2, eps: as eigen_trainer_adam.
 *   weight_decay: chainer's AdamRule weight_decay_rate with eta = 1: p -= lr_t m / (sqrt(v) + eps) + weight_decay p, the two terms
 *     added first and then subtracted.  0: off.
 *   clip_norm: chainer's GradientClipping: with norm the global L2 norm of the gradient table, the step uses g' = rate g,
 *     rate = (float)(clip_norm / norm) (divided in double) where norm > clip_norm, else 1.  0: off.  The gradient table itself is
 *     not modified: eigen_trainer_get_grads still returns g.  A norm of exactly 0 gives rate 1; nothing divides by it.
 *   skip_nonfinite: 1: a step whose norm is not finite is not taken (see the entry).  reserved: 0. */
typedef struct {
    double alpha, beta1, beta2, eps, weight_decay, clip_norm;
    int32_t skip_nonfinite, reserved;
} eigen_adam_settings;

/* What a step did: the global norm it saw, the rate it applied (in double: clip_norm / norm, or 1) and whether it was applied. */
typedef struct {
    double norm, rate;
    int32_t applied, reserved;
} eigen_adam_report;

/* The L2 norms of the current gradient table: *h_global that of all tensors together, h_per_tensor[k] that of tensor k in
 * eigen_set_prednet_weights order (n_tensors of them).  Either output may be NULL.  Per tensor the squares are summed in double
 * (a float's square is exact there): NORM_SLICES fixed strided slices, a fixed tree within each, the slices added in order; the
 * global norm is the square root of the tensors' sums added in tensor order.  A norm that is not finite is a value to return,
 * not an error.  The call synchronises the stream when it has an output to write.
 * Errors: EIGEN_ERR_INVALID a NULL handle, n_tensors not the handle's count; EIGEN_ERR_STATE no weights. */
int eigen_trainer_grad_norms(eigen_trainer* t, double* h_global, double* h_per_tensor, int32_t n_tensors, void* stream);

/* One Adam step under `settings`.  With weight_decay = 0, clip_norm = 0, skip_nonfinite = 0 and h_report = NULL it launches exactly
 * what eigen_trainer_adam launches, hence the same bits.  Otherwise it computes the norms on the device (as
 * eigen_trainer_grad_norms) and runs the clipped, decayed update, which reads the norm from device memory: a clipped step needs no
 * host round trip.  With skip_nonfinite the call reads the norm back first, which synchronises the stream; if it is not finite
 * nothing is changed (weights, moments and the step count stay as they are) and the report says applied = 0.  With a report and
 * without skip_nonfinite the norm is read back after the launch.  WITHOUT skip_nonfinite A GRADIENT THAT IS NOT FINITE IS APPLIED, as
 * eigen_trainer_adam applies it: the weights it reaches are lost.
 * Errors, before any launch: EIGEN_ERR_INVALID a NULL handle or settings, weight_decay or clip_norm negative or not finite,
 * skip_nonfinite not 0 or 1, reserved not 0, and what eigen_trainer_adam refuses for alpha, beta1, beta2, eps; EIGEN_ERR_STATE no
 * weights. */
int eigen_trainer_adam_ex(eigen_trainer* t, const eigen_adam_settings* settings, eigen_adam_report* h_report, void* stream);

/* The gradient accumulator: a second table of the gradient's size, on the device, which sums the gradients of several
 * eigen_trainer_loss_grad* calls (each of which overwrites the gradient table) into one step: micro-batches of a logical batch the
 * tape cannot hold, or terms under different objectives.
 *   EIGEN_ACC_ADD: acc[i] = acc[i] + s g[i] with s = (float)scale, one rounded product and one rounded sum; on an empty
 *     accumulator the sum starts from zero.
 *   EIGEN_ACC_LOAD: the gradient table becomes a copy of the accumulator, which keeps its contents.
 *   EIGEN_ACC_CLEAR: the accumulator is zeroed and empty again.  `scale` is read by ADD alone.
 * The table is made by the first ADD; eigen_trainer_tape_bytes does not count it.  eigen_trainer_set_weights discards what was
 * accumulated, and the accumulator is no part of eigen_trainer_get_state / _set_state: a checkpoint is taken between steps.
 * Errors, before any launch: EIGEN_ERR_INVALID a NULL handle, an unknown op, a scale that is not finite; EIGEN_ERR_STATE no weights,
 * EIGEN_ACC_LOAD with nothing accumulated. */
enum { EIGEN_ACC_CLEAR = 0, EIGEN_ACC_ADD = 1, EIGEN_ACC_LOAD = 2 };
int eigen_trainer_accumulate(eigen_trainer* t, int32_t op, double scale, void* stream);

/* Device bytes of the handle's tape (activations kept for the backward pass) at max_batch x max_steps. */
int64_t eigen_trainer_tape_bytes(const eigen_trainer* t);

/* ---------------------------------------------------------------------------------------------------- dense fitness
 * The dense motion score on the population path: the score EIGEN_OBJ_FLOW climbs, as the fitness of a genome.
 * It needs an inference handle only: no trainer, no tape.  For every sample the stage takes two emitted uint8 frames img0 (the
 * reference) and img1 and does what eigen_trainer_flow_term_pair does on the float images (float)byte / 255.0f of the two, img1 as the
 * prediction and img0 as d_prev: the gray planes, the normalised Scharr pair of I0, It = I1 - I0, the five truncated window sums, the
 * 2x2 solve with eps on the diagonal, the field u in float64, and then the two moment passes of the chosen score (for Free with the
 * prepare and pair passes between them), in the operations and orders of csrc/flow_obj_kernels.h, flow_score_kernels.h and
 * flow_struct_kernels.h.  The fitness of a sample is S_b, entry 8 of its own record; a sample with fewer than min_count members scores
 * exactly 0.  Float64, one IEEE operation per operation written, fixed partitions and orders, no float atomics: the result of a
 * sample does not depend on the batch it is in.  No seed, q or gradient is formed, and no corner, Lucas-Kanade or score_kernel launch
 * happens.
 *   flow: radius and eps as eigen_trainer_flow_term reads them; flags must be 0 (the eval entries also take EIGEN_DENSE_FLOAT_FRAMES,
 *   below).  Exactly one of score (Circles, CirclesFree) and
 *   sscore (Bands, Free) is non-NULL.
 * The workspace, seven float64 planes of max_batch * H * W and one byte plane, is allocated by the first dense call on the handle, all
 * of it or none, and freed with the handle. */
typedef struct {
    eigen_flow_settings flow;
    const eigen_flow_score* score;
    const eigen_flow_structure_score* sscore;
} eigen_dense_settings;

/* The stage alone on two batches of byte images, as eigen_flow is for Lucas-Kanade: image b at d_imgX + b * strideX (bytes), planar
 * [C][H][W]; bytes between the images are never read.  d_mask: uint8 [H][W] shared by the batch, 0 = the pixel is no member, or NULL.
 * Outputs, each may be NULL: h_fitness host double[batch], S_b; h_stats host double[batch][10], the records (eigen_trainer_flow_term_score
 * / eigen_trainer_flow_term_structure state their entries); d_flow device double [batch][2][H][W], the field u.  The call synchronises
 * the stream when it has a host output to write.
 * Errors, before any launch, all EIGEN_ERR_INVALID: a NULL handle, image or settings, batch < 1 or above max_batch, a stride below
 * C*H*W, both scores or neither, and what eigen_trainer_flow_term_score / _structure refuse for the radius, eps, flags, the mask and the
 * score's fields, in their words. */
int eigen_dense_score(eigen_engine* e, const uint8_t* d_img0, int64_t stride0, const uint8_t* d_img1, int64_t stride1, int32_t batch,
                      const eigen_dense_settings* settings, const uint8_t* d_mask, double* h_fitness, double* h_stats, double* d_flow,
                      void* stream);

/* eigen_eval_population with the dense stage in place of flow and score: render -> roll-out -> eigen_dense_score on the two frames
 * the pairing names (POPULATION: the prediction after step n_repeat is img0, the first extension frame img1; SINGLE: the input image
 * is img0, the second extension frame img1).  h_fitness: host double[n_genomes], required; h_stats: host double[n_genomes][10] or NULL.
 * structure must be the one the settings' score belongs to: EIGEN_BANDS / EIGEN_FREE the sscore of that structure, EIGEN_CIRCLES /
 * EIGEN_CIRCLES_FREE the score.  eigen_get_timings then reports the dense stage as [2] and 0 as [3].
 * Errors: as eigen_eval_population and eigen_dense_score (a batch above max_batch is EIGEN_ERR_INVALID here too); EIGEN_ERR_INVALID a
 * structure the settings' score does not belong to.  The structure, the pairing (n_ext), the batch and the settings are refused before
 * the workspace is allocated and before the render; what eigen_render_cppn and eigen_prednet_rollout themselves refuse (no grid, no
 * weights, a malformed genome) comes from them, as in eigen_eval_population. */
int eigen_eval_population_dense(eigen_engine* e, const eigen_genome_batch* h_genomes, int32_t structure, int32_t bg, int32_t gradient,
                                int32_t pairing, const eigen_dense_settings* settings, const uint8_t* d_mask, double* h_fitness,
                                double* h_stats, void* stream);

/* eigen_eval_images likewise, for ready-made images (there are no vectors and counts to return). */
int eigen_eval_images_dense(eigen_engine* e, const uint8_t* d_images, int32_t batch, int32_t structure, int32_t pairing,
                            const eigen_dense_settings* settings, const uint8_t* d_mask, double* h_fitness, double* h_stats, void* stream);

/* ---------------------------------------------------------------------------------------------------- dense fitness: the solve
 * The opt-in solve of the dense stage ("The pyramidal, iterated solve"; csrc/dense_pyr_kernels.h): Lucas-Kanade
 * over `levels` pyramid levels with `iters` iterations per level in the per-pixel window form, in place of the single regularised
 * step.  Score only: no gradient, no trainer entry.  Float64, one IEEE operation per operation written, fixed orders.
 *   gray planes  I0, I1 of level 0 are what the single step reads: the gray of (float)byte / 255.0f, widened.
 *   pyramid      level l + 1 has size ((W_l + 1) / 2, (H_l + 1) / 2).  5 taps (1, 4, 6, 4, 1) / 16 centred on source index 2 i, reflect-101
 *                borders, along x first (at every source row), then along y; one tap set is (((a + e) + 4.0 (b + d)) + 6.0 c) / 16.0.
 *                Both images are reduced.
 *   per level    from the coarsest to the finest: Ix, Iy the normalised Scharr pair of the level's I0, indices clamped; Gxx, Gxy, Gyy the
 *                truncated window sums in the single step's order (rows first, then columns, offsets ascending, each sum started from
 *                its first term); a = Gxx + eps, c = Gyy + eps, b = Gxy, det = a c - b b.  They do not change over the iterations.
 *   start        the coarsest level starts from the zero field, held as -0.0 so that the first step added to it is the step itself bit
 *                for bit (a step of -0.0 included); otherwise u_l(y, x) = 2.0 u_{l+1}(y >> 1, x >> 1), both components.
 *   iteration    at pixel p with its own u = (ux, uy), for every q of the truncated window of p: d(q) = S(I1, qx + ux, qy + uy) - I0(q);
 *                bx = sum Ix(q) d(q), by = sum Iy(q) d(q), per window row ascending in x from its first term, then the rows ascending
 *                in y from the first row; ux += -((c bx - b by) / det), uy += -((a by - b bx) / det).
 *   sampler S    x = x > 0 ? x : 0, then x = x < W - 1 ? x : W - 1, likewise y; x0 = floor(x), x1 = min(x0 + 1, W - 1), fx = x - x0,
 *                likewise y; top = v00 + fx (v01 - v00), bot = v10 + fx (v11 - v10), S = top + fy (bot - top).  At integer coordinates S
 *                is the pixel exactly, so levels = 1, iters = 1 through the iteration kernel is the single step's field bit for bit.
 *   score        the field of level 0 after its last iteration goes into the unchanged moment, prepare, pair and final kernels: the
 *                records and S_b keep their meaning, and a sample's result still does not depend on its batch.
 * Accepted: levels 1 .. 6, iters 1 .. 32, and a coarsest level of at least 4 pixels on its shorter side; anything else is
 * EIGEN_ERR_INVALID before any launch or allocation.  The pyramid (four float64 planes per pixel of every level, at max_batch) is
 * allocated by the first iterated call on the handle, all of it or none, and freed with the handle; a handle that never asks
 * allocates nothing more than before. */
typedef struct {
    int32_t levels;
    int32_t iters;
} eigen_dense_solve;

/* The three dense entries with a solve.  solve NULL or {1, 1}: the call is the namesake's, launch for launch (the namesakes are these
 * entries with NULL).  Errors: the namesake's, and EIGEN_ERR_INVALID for a solve outside the accepted values.  eigen_get_timings
 * reports the stage as the namesakes do. */
int eigen_dense_score_iter(eigen_engine* e, const uint8_t* d_img0, int64_t stride0, const uint8_t* d_img1, int64_t stride1, int32_t batch,
                           const eigen_dense_settings* settings, const uint8_t* d_mask, double* h_fitness, double* h_stats, double* d_flow,
                           void* stream, const eigen_dense_solve* solve);
int eigen_eval_population_dense_iter(eigen_engine* e, const eigen_genome_batch* h_genomes, int32_t structure, int32_t bg, int32_t gradient,
                                     int32_t pairing, const eigen_dense_settings* settings, const uint8_t* d_mask, double* h_fitness,
                                     double* h_stats, void* stream, const eigen_dense_solve* solve);
int eigen_eval_images_dense_iter(eigen_engine* e, const uint8_t* d_images, int32_t batch, int32_t structure, int32_t pairing,
                                 const eigen_dense_settings* settings, const uint8_t* d_mask, double* h_fitness, double* h_stats, void* stream,
                                 const eigen_dense_solve* solve);

/* ---------------------------------------------------------------------------------------------------- dense fitness: members
 * The three dense entries with members ("Members"; csrc/dense_member_kernels.h): each takes its _iter namesake's
 * arguments plus an eigen_flow_members, the struct of the trainer's scores.  members NULL: the call is the namesake's, launch for launch.
 *   EIGEN_FLOW_MEMBERS_CORNERS: the members of sample b are the corners picked on img0 of its pair, the image the solve treats as the
 *     reference, by cvtColor / cornerMinEigenVal(block_size, 3) / goodFeaturesToTrack(max_corners, quality_level, min_distance) with
 *     eigen_flow's own kernels, in the sequence of the trainer's membership stage; d_mask, if given, is the shared [H][W] plane and
 *     removes the corners it does not count.  The member planes [B][H W] then take the mask's place in the unchanged moment, prepare and
 *     final kernels.
 *   EIGEN_FLOW_MEMBERS_MASK: d_mask holds one plane per sample, mask_bstride >= H*W bytes apart.  A plane set that counts no pixel at
 *     all is refused; a single sample that counts none scores exactly 0.
 * Members change who is counted, never the solve: the field is the single step's or the levels x iters solve's.  The record of a call
 * with corner members is, bit for bit, that of eigen_trainer_flow_term_pair with the same members on the (float)byte / 255.0f images.
 * Under members the Free structure's pair pass runs over a compacted list of the members (at most max_corners, or H*W under planes)
 * and leaves the bytes the all-pixel pass leaves for the same members.
 * The workspace (the corner buffers of the trainer's membership stage; for Free the list, 12 bytes per slot of max_batch times the
 * slots of a sample) is made by the first call that needs it, all of a group or none, and freed with the handle; a handle that never
 * passes members allocates nothing more than before.  eigen_get_timings reports the stage, the membership stage included, as [2].
 * eigen_dense_score_members: h_members (host, may be NULL) receives uint8 [batch][H][W], the member planes, and h_counts (host, may be
 * NULL) int32 [batch], the corners selected per sample before the mask, as eigen_trainer_flow_members gives them; both are written under
 * CORNERS only.
 * Errors: the namesake's; EIGEN_ERR_INVALID before any launch or allocation, with the outputs untouched, for what
 * eigen_trainer_flow_term_members refuses of the members, in its words: an unknown kind, reserved != 0, max_corners outside 1 .. 128,
 * block_size outside 1 .. 9, quality_level outside (0, 1], min_distance negative or not finite, mask_bstride below H*W under MASK or
 * not 0 under CORNERS, MASK without d_mask, a plane set that counts no pixel. */
int eigen_dense_score_members(eigen_engine* e, const uint8_t* d_img0, int64_t stride0, const uint8_t* d_img1, int64_t stride1, int32_t batch,
                              const eigen_dense_settings* settings, const uint8_t* d_mask, double* h_fitness, double* h_stats, double* d_flow,
                              void* stream, const eigen_dense_solve* solve, const eigen_flow_members* members, uint8_t* h_members,
                              int32_t* h_counts);
int eigen_eval_population_dense_members(eigen_engine* e, const eigen_genome_batch* h_genomes, int32_t structure, int32_t bg, int32_t gradient,
                                        int32_t pairing, const eigen_dense_settings* settings, const uint8_t* d_mask, double* h_fitness,
                                        double* h_stats, void* stream, const eigen_dense_solve* solve, const eigen_flow_members* members);
int eigen_eval_images_dense_members(eigen_engine* e, const uint8_t* d_images, int32_t batch, int32_t structure, int32_t pairing,
                                    const eigen_dense_settings* settings, const uint8_t* d_mask, double* h_fitness, double* h_stats,
                                    void* stream, const eigen_dense_solve* solve, const eigen_flow_members* members);

/* ---------------------------------------------------------------------------------------------------- dense fitness: float frames
 * The dense stage on PredNet's float predictions in place of the bytes the roll-out emits ("Float frames";
 * csrc/dense_float_kernels.h): the image pair the flow objective itself is evaluated on, so that the fitness is a continuous function
 * of the network's output between its norm cuts.  Bit 1 of eigen_dense_settings.flow.flags; the six eigen_eval_population_dense* /
 * eigen_eval_images_dense* entries accept 0 or this bit, and refuse every other bit as before.  The three byte-stage entries
 * eigen_dense_score* refuse it and name eigen_dense_score_float.
 *   EIGEN_PAIR_POPULATION: img0 = P0 after step n_repeat, img1 = P0 after the first extension step, both float32 [C0][H][W] as ConvP0
 *     wrote them: clamped to [0, 1], before the byte.
 *   EIGEN_PAIR_SINGLE: img0 is the input image, (float)byte / 255.0f as without the flag; img1 = P0 after the second extension step.
 * The roll-out itself does not change by a bit: extension steps are fed as cfg.requant_feedback says and the emitted frames are the
 * bytes a call without the flag emits.  One launch behind the ConvP0 launch of a named step writes the float64 gray plane of P0
 * (tflow_gray's operations on the widened float32 values); the stage starts from the two gray planes I0, I1 [B][H W], forms the
 * normalised Scharr pair of I0 and It = I1 - I0 from them, and launches the single step or the levels x iters solve, the score passes
 * and the members exactly as they are.  Hence the record of a sample is, bit for bit, the record eigen_trainer_flow_term_pair (for a
 * byte img0: eigen_trainer_flow_term) leaves on the same float images under the same score, mask, members and solve; on float images
 * that are exactly (float)byte / 255.0f it is the record eigen_dense_score leaves on those bytes.  Corner members are picked on the
 * byte image of img0, (uint8)(int)(v * 255.0f): on the population path the emitted frame (or the input image), so the corners are
 * the ones the byte fitness and the sparse fitness pick.
 * Workspace: under the single step two float64 planes of max_batch * H * W; the iterated solve keeps the planes as level 0 of its
 * pyramid.  The first float call on the handle allocates it, behind every refusal and before the render and the roll-out, and it is
 * freed with the handle; a handle that never asks allocates nothing new. */
#define EIGEN_DENSE_FLOAT_FRAMES 2

/* The float stage alone.  Exactly one of d_img0 (uint8) and d_fimg0 (float32) is non-NULL, the d_ref / d_fref convention of the
 * trainer's entries; d_img1 is float32.  Image b at its pointer + b * its stride, strides in elements, planar [C][H][W]; float values
 * are read as they are (the corner members clamp them to [0, 1] for the byte).  settings->flow.flags is 0 or
 * EIGEN_DENSE_FLOAT_FRAMES; solve and members may be NULL.  Outputs and synchronisation as eigen_dense_score.  With a float img0
 * under corner members the handle keeps one byte copy of max_batch images, made by the first such call.
 * Errors: eigen_dense_score_members' own, in its words, and EIGEN_ERR_INVALID for both or neither img0; all before any launch. */
int eigen_dense_score_float(eigen_engine* e, const uint8_t* d_img0, const float* d_fimg0, int64_t stride0, const float* d_img1, int64_t stride1,
                            int32_t batch, const eigen_dense_settings* settings, const eigen_dense_solve* solve, const eigen_flow_members* members,
                            const uint8_t* d_mask, double* h_fitness, double* h_stats, double* d_flow, void* stream);

/* Stage-level read-back for the tests: the two gray planes of the last float dense call on the handle, host double [batch][H][W] each.
 * EIGEN_ERR_STATE where there was none (or an iterated byte call has since overwritten level 0 of the pyramid), or where the batch
 * differs.  It launches no kernel. */
int eigen_debug_dense_gray(eigen_engine* e, int32_t batch, double* h_I0, double* h_I1, void* stream);

/* Test hook of the solve: force >= 0 sets whether levels = 1, iters = 1 (and a NULL solve) goes through the iteration kernel too, on
 * this handle; pyramid_bytes (may be NULL) receives the bytes of the pyramid the handle holds, 0 before its first iterated call. */
int eigen_debug_dense_solve(eigen_engine* e, int32_t force, int64_t* pyramid_bytes);

/* ---- The flow objective through the solve ("The iterated solve's gradient").  With a solve of more than one level or
 * iteration the flow stage of a term runs eigen_dense_solve's semantics on the trainer's float images (I0 the gray of the reference, I1 the
 * gray of the prediction, as the single step's planes form them; on floats that are exactly (float)byte / 255.0f the field is
 * eigen_dense_score_iter's d_flow bit for bit), the unchanged value / score / members kernels read the field of level 0, and the seed and
 * the reference gradient are the exact derivative of the written formulas through every iteration and level, with floor,
 * x1 = min(x0 + 1, W - 1) and the sampler's two clamps held constant (a clamped coordinate passes no gradient).  Float64, fixed orders, no
 * atomics; cast to float once where the single step's seed and reference gradient are stored or added.
 * The workspace (pyramid, every iterate and the adjoint planes, at max_batch) is allocated by the first iterated call on the handle, all
 * of it or none, and freed with the handle; a handle that never asks allocates nothing more than before.
 *
 * eigen_trainer_flow_term_iter: eigen_trainer_flow_term_members' arguments (at most one of score and sscore; neither: the displacement
 * modes, which take d_dir) plus d_dir and solve.  eigen_trainer_loss_grad_flow_iter: eigen_trainer_loss_grad_flow_members' arguments plus
 * solve; both pairings and EIGEN_FLOW_MOVING_REFERENCE are accepted.  solve NULL or {1, 1}: the call is its namesake's (or, without a
 * score, eigen_trainer_flow_term / _ref / _pair's), launch for launch and bit for bit.
 * Errors: the namesakes'; EIGEN_ERR_INVALID before any launch or allocation for a solve outside eigen_dense_solve's accepted values
 * (levels 1 .. 6, iters 1 .. 32, a coarsest level of at least 4 pixels), in that struct's own words. */
int eigen_trainer_flow_term_iter(eigen_trainer* t, const float* d_pred, int64_t p_bstride, const uint8_t* d_ref, const float* d_fref,
                                 int64_t r_bstride, int32_t batch, const eigen_flow_settings* flow, const uint8_t* d_mask,
                                 const eigen_flow_score* score, const eigen_flow_structure_score* sscore, const eigen_flow_members* members,
                                 double scale, double* h_value, double* h_stats, double* d_flow, float* d_seed, int64_t s_bstride,
                                 float* d_ref_grad, int64_t rg_bstride, void* stream, const float* d_dir, const eigen_dense_solve* solve);
int eigen_trainer_loss_grad_flow_iter(eigen_trainer* t, const uint8_t* d_frames, int64_t bstride, int32_t batch, int32_t n_steps,
                                      int32_t n_fed, int32_t requant, int32_t reset, const double* h_step_w, int32_t objective,
                                      const double* h_layer_w, double* h_loss, double* h_layer_err, float* d_pred, float* d_frame_grad,
                                      int64_t g_bstride, int64_t g_tstride, const eigen_flow_settings* flow, const float* d_dir,
                                      const uint8_t* d_mask, double* h_terms, int32_t pairing, const eigen_flow_score* score,
                                      const eigen_flow_structure_score* sscore, const eigen_flow_members* members, double* h_stats,
                                      void* stream, const eigen_dense_solve* solve);

/* Test hook of the trainer's solve: force >= 0 sets whether a {1, 1} (or NULL) solve goes through the iterated stage and its backward
 * too, on this handle; workspace_bytes (may be NULL) receives the bytes of the iterated workspace the handle holds, 0 before its first
 * iterated call. */
int eigen_trainer_debug_flow_iter(eigen_trainer* t, int32_t force, int64_t* workspace_bytes);

/* ---- The flow objective against a target field ("The target field"): a third displacement mode, the squared
 * endpoint error of the solved field u against a per-call field, in u's own sign convention (content at x in the reference is at x + u in
 * the prediction; eigen_render_moving_cppn states its flow the same way).  Float64, one IEEE operation per operation written:
 *   ex = ux - tx, ey = uy - ty, v = ex ex + ey ey, g = (2 ex, 2 ey); where the mask does not count the pixel v = 0 and g = 0
 * and the term is sum(v) / (B N_m) through the displacement modes' own fixed-order reduction; kappa keeps their divisor.  q is formed from
 * g over the solve's a, b, c and det in the solve's written formula; the seed, the reference gradient, the moving reference, both pairings
 * and the gradient through an iterated solve are the other displacement modes'.  The target is device data and is not inspected: a
 * non-finite element propagates.
 *
 * eigen_trainer_flow_term_target: eigen_trainer_flow_term_iter's arguments plus d_target, doubles [B][2][H W], sample b at
 * d_target + b * t_bstride.  eigen_trainer_loss_grad_flow_target: eigen_trainer_loss_grad_flow_iter's arguments plus d_target, t_bstride
 * and t_tstride: term s (prediction P0_s) reads d_target + b * t_bstride + s * t_tstride.  d_target NULL: the call is its _iter namesake,
 * launch for launch and bit for bit, the strides are not read and nothing is allocated.
 * Errors: the namesakes'; EIGEN_ERR_INVALID before any launch or allocation for a target together with score, sscore, members or d_dir,
 * for t_bstride < 2 H W, for t_tstride < 2 H W when n_steps > 2, and for a target under an objective other than EIGEN_OBJ_FLOW. */
int eigen_trainer_flow_term_target(eigen_trainer* t, const float* d_pred, int64_t p_bstride, const uint8_t* d_ref, const float* d_fref,
                                   int64_t r_bstride, int32_t batch, const eigen_flow_settings* flow, const uint8_t* d_mask,
                                   const eigen_flow_score* score, const eigen_flow_structure_score* sscore, const eigen_flow_members* members,
                                   double scale, double* h_value, double* h_stats, double* d_flow, float* d_seed, int64_t s_bstride,
                                   float* d_ref_grad, int64_t rg_bstride, void* stream, const float* d_dir, const eigen_dense_solve* solve,
                                   const double* d_target, int64_t t_bstride);
int eigen_trainer_loss_grad_flow_target(eigen_trainer* t, const uint8_t* d_frames, int64_t bstride, int32_t batch, int32_t n_steps,
                                        int32_t n_fed, int32_t requant, int32_t reset, const double* h_step_w, int32_t objective,
                                        const double* h_layer_w, double* h_loss, double* h_layer_err, float* d_pred, float* d_frame_grad,
                                        int64_t g_bstride, int64_t g_tstride, const eigen_flow_settings* flow, const float* d_dir,
                                        const uint8_t* d_mask, double* h_terms, int32_t pairing, const eigen_flow_score* score,
                                        const eigen_flow_structure_score* sscore, const eigen_flow_members* members, double* h_stats,
                                        void* stream, const eigen_dense_solve* solve, const double* d_target, int64_t t_bstride,
                                        int64_t t_tstride);

/* ---- The joint objective and the valid pixels ("The joint objective and the valid pixels").
 *
 * Validity planes under a target field: sample b of a term has a byte plane V_b [H W]; a pixel counts where the shared mask M counts it
 * (all pixels without one; N_m is its count) and V_b is not zero.  With c_b the integer count of the counted pixels of sample b and
 * r_b = c_b > 0 ? (double)N_m / (double)c_b : 0.0, in float64, one IEEE operation per operation written:
 *   ex, ey, v as under the target field; mv = counted ? v r_b : 0, g = counted ? ((2 ex) r_b, (2 ey) r_b) : 0
 * and everything behind mv and g is the target field's own (the fixed-order sum, the division by B N_m, kappa, q, the seed, the reference
 * path, the gradient through an iterated solve).  The term is the mean over the samples of each sample's mean squared endpoint error
 * over its own counted pixels; a sample that counts no pixel contributes exactly 0 and a zero gradient; planes that are all ones give
 * r_b = 1.0 exactly and the bytes of the call without planes.  The counts are summed without atomics.
 *
 * eigen_trainer_flow_term_valid: eigen_trainer_flow_term_target's arguments plus d_valid, bytes, sample b at d_valid + b * v_bstride as
 * [H W] (NULL: the call is its _target namesake, launch for launch).
 *
 * The joint objective: loss = L_flow + frame_weight * L_mse, where L_flow is the loss of the same call without a frame weight and L_mse
 * the squared error of the image-layer predictions against the next frames under the call's own step weights, reduced as the
 * EIGEN_OBJ_MSE call with the same step weights reduces it.  Term s seeds d loss / d P0_s with the flow term's seed plus
 * (float)(frame_weight * the squared error's scale of step s, formed in double) * (P0_s - x_{s+1}); a frame gradient holds the input path,
 * the flow terms' reference paths under EIGEN_FLOW_MOVING_REFERENCE and frame_weight times the squared error's target path.  The frame
 * term goes with every mode, score, members setting, solve, pairing and reference of the flow objective.
 *
 * eigen_trainer_loss_grad_flow_joint: eigen_trainer_loss_grad_flow_target's arguments plus `joint` (NULL: the call is its _target
 * namesake, launch for launch and bit for bit).  Term s (prediction P0_s) reads the plane of sample b at
 * d_valid + b * v_bstride + s * v_tstride.
 * Errors: the namesakes'; EIGEN_ERR_INVALID before any launch or allocation for a frame_weight that is negative or not finite, for a
 * frame_weight > 0 under an objective other than EIGEN_OBJ_FLOW, for d_valid without d_target, for v_bstride < H W, and for
 * v_tstride < H W when n_steps > 2.  After a refusal the outputs are untouched and the handle still works. */
typedef struct eigen_flow_joint {
    double frame_weight;      /* mu >= 0; 0: no frame term */
    const uint8_t* d_valid;   /* device validity planes, or NULL */
    int64_t v_bstride;        /* bytes between two samples' planes, >= H W */
    int64_t v_tstride;        /* bytes between two terms' planes, >= H W when n_steps > 2 */
    double* h_parts;          /* host, two doubles out: L_flow, L_mse; may be NULL */
} eigen_flow_joint;

int eigen_trainer_flow_term_valid(eigen_trainer* t, const float* d_pred, int64_t p_bstride, const uint8_t* d_ref, const float* d_fref,
                                  int64_t r_bstride, int32_t batch, const eigen_flow_settings* flow, const uint8_t* d_mask,
                                  const eigen_flow_score* score, const eigen_flow_structure_score* sscore, const eigen_flow_members* members,
                                  double scale, double* h_value, double* h_stats, double* d_flow, float* d_seed, int64_t s_bstride,
                                  float* d_ref_grad, int64_t rg_bstride, void* stream, const float* d_dir, const eigen_dense_solve* solve,
                                  const double* d_target, int64_t t_bstride, const uint8_t* d_valid, int64_t v_bstride);
int eigen_trainer_loss_grad_flow_joint(eigen_trainer* t, const uint8_t* d_frames, int64_t bstride, int32_t batch, int32_t n_steps,
                                       int32_t n_fed, int32_t requant, int32_t reset, const double* h_step_w, int32_t objective,
                                       const double* h_layer_w, double* h_loss, double* h_layer_err, float* d_pred, float* d_frame_grad,
                                       int64_t g_bstride, int64_t g_tstride, const eigen_flow_settings* flow, const float* d_dir,
                                       const uint8_t* d_mask, double* h_terms, int32_t pairing, const eigen_flow_score* score,
                                       const eigen_flow_structure_score* sscore, const eigen_flow_members* members, double* h_stats,
                                       void* stream, const eigen_dense_solve* solve, const double* d_target, int64_t t_bstride,
                                       int64_t t_tstride, const eigen_flow_joint* joint);

#ifdef __cplusplus
}
#endif
#endif /* EIGEN_ENGINE_H */
