/*
 * epnn.h -- C ABI of libepnn_hip.so, the MI355X (gfx950) implementation of the EPNN hot path.
 *
 * The reference (derekmetcalf/epnn) has no FFI: its "operator API" for this path is the Python/Keras layer
 * interface of charge_gn.py.  Each entry point below names the reference interface it stands in for; the
 * Python mirror of that interface (epnn_amd/charge_gn.py) binds these symbols with ctypes and nothing else.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; epnn_last_error() gives the message of the
 *     last failing call on the calling thread.
 *   - all tensors are float32, row-major, caller-owned.  "host" entry points take host pointers and copy;
 *     "_dev" entry points take pointers obtained from epnn_dev_alloc() on the same handle and run
 *     asynchronously on the handle's stream (epnn_sync() waits).
 *   - one handle per device; calls on one handle must be serialised by the caller.
 *   - flat ("ragged") molecule batches: B molecules, molecule b owns atoms [offsets[b], offsets[b+1]) of the
 *     flat atom arrays; N is the padded atom count the reference would have used (gen_padded_init_state pads
 *     every molecule to the directory maximum, charge_gn.py:340-364).  N enters the arithmetic: the reference
 *     sums messages over all N partners including the padded ones (charge_gn.py:70).
 *   - arithmetic: float32-grade throughout, like the reference's (TensorFlow float32).  The inference kernels run the Dense layers
 *     of the pair and update MLPs on the bf16 matrix pipe as six bf16 products of EXACT three-piece splits of both operands per product (what is
 *     left out is below 2^-24 of a product, the rounding of an f32 multiply-add); results agree with a
 *     float64 evaluation of the reference's algorithm to float32 rounding noise (1e-7 .. 1e-6 on the charges).  Every sum has a
 *     fixed order: results are bit-reproducible and independent of batch composition and of sharding.  The fused kernel of the compact
 *     entry runs its pair MLPs on operands scaled by 2^-32 (the first ReLU is then the output clamp of the add in front of it, and the
 *     linear map behind the pair MLP is scaled by 2^32): a power of two changes no mantissa, so the charges are the unscaled
 *     arithmetic's bit for bit while the pair MLPs' first-layer inputs stay between 2^-70 and 2^31 in magnitude; a molecule's step whose
 *     rows are larger runs with the plain ReLU by itself (counted in epnn_last_stats out[3]), values smaller than that are float32
 *     rounding noise of the sums they enter.
 */
#ifndef EPNN_H
#define EPNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct epnn_handle epnn_handle;

/* Hyper-parameters fixed at make_model time (charge_gn.py:369-374, 413-418) and the featuriser constants of
 * get_init_edges (charge_gn.py:122: cutoff=3.0, eta=2.0, mu=linspace(0.1,cutoff,e_dim)); near_tol is the
 * 1e-5 of EPN_layer.call (charge_gn.py:90). */
typedef struct epnn_config {
    int32_t nx;       /* atom feature columns: 9 (infer.py table) or 10 (charge_gn.py table)          */
    int32_t h_dim;    /* channels of h, 1..48 (48 in the reference's scripts; must equal e_dim, charge_gn.py:377) */
    int32_t e_dim;    /* channels of e = Gaussians of get_init_edges, == h_dim                         */
    int32_t T;        /* message / electron passing steps, 1..8                                        */
    int32_t hidden;   /* 32: hidden width of every MLP and the message width (charge_gn.py:52,84,415)  */
    float cutoff;     /* 3.0                                                                           */
    float eta;        /* 2.0                                                                           */
    float near_tol;   /* 1e-5                                                                          */
} epnn_config;

enum { EPNN_W_MSG = 0, EPNN_W_UPD = 1, EPNN_W_PAS = 2 };

const char *epnn_last_error(void);
int epnn_version(void);
/* number of HIP devices visible (0 when there is none; never initialises a context beyond the count). */
int epnn_device_count(void);

/* make_model (charge_gn.py:369-391): creates the layer stack on `device`.  Weights start at zero.
 *
 * CONTRACT -- what of the reference's constructor arguments is free and what is fixed.  In the reference `layers` sizes the UPDATE
 * MLP only (make_model: MLP_layer(layers, out_dim=h_dim), charge_gn.py:371); the message and pass MLPs are ([32, 32], 32) and
 * ([32, 32], 1) by its own constants (:52, :84), and every width follows h_dim (:369-374).  Every checkpoint it ships and both of
 * its scripts use layers = [32, 32], h_dim = e_dim = 48 (:413-417, infer.py:47-50).
 *   free :  nx in 1..10 (atom feature columns; 9 and 10 are the reference's two tables; up to 13 on the fused kernels alone:
 *           epnn_create_fused), T in 1..8, cutoff, eta, near_tol,
 *           h_dim = e_dim in 1..48 (below 48 the model runs as a 48-channel one: zero channels of h and e, zero rows / columns of
 *           the kernels that touch them -- exact, the padding feeds nothing, stays zero through every step and has zero gradient;
 *           every weight, tensor and epnn_edges row at this interface has the MODEL's h_dim channels),
 *           the padded size N and the batch size of every call, every weight value; `layers` of the update MLP (1..7 hidden
 *           layers of 1..256 units each: epnn_set_update_layers) for every inference entry and the training step;
 *   fixed:  hidden == 32 (the reference's own constant for the message / pass MLPs), h_dim == e_dim (make_model gives e_inp h_dim
 *           channels, charge_gn.py:377) and at most 48 (the kernels' register / LDS layouts hold 48 channels).
 * epnn_create FAILS (returns non-zero, epnn_last_error says which field) for any other value.  `layers` == [32, 32] runs the
 * kernels DESIGN.md describes, and so does every `layers` of one or two hidden layers of at most 32 units: the library runs it as a
 * [32, 32] model on a zero-padded copy of its weights (units with zero weights and bias feed nothing; a missing second layer is the
 * identity on the first layer's non-negative outputs) -- exact, not an approximation.  One or two hidden layers of at most 64
 * units run molecules of up to 32 atoms on a 64-unit build of the fused kernel (the same embedding into [64, 64]; 181 M atoms/s on
 * the bench batch against 274 M for [32, 32]) and larger ones through the tiled kernels with one launch per stage and a generic
 * (f32 FMA) Dense stack as the update stage; any other `layers` (a width above 64, three or more hidden layers) runs every molecule
 * that way (28 M atoms/s on the bench batch: tools/bench_layers.py).  The training step of any `layers` but [32, 32] runs one launch per Dense layer ("train_fused" = 0's kernels)
 * on the model's own shapes -- the same results to float32 rounding, several times slower per small molecule. */
int epnn_create(const epnn_config *cfg, int device, epnn_handle **out);
/* The same with nx in 1..13: what the fused kernels' operand of (node mask, x, charge, one) holds, nx + 3 <= 16.  A handle with
 * nx > 10 runs on the fused kernels ONLY: epnn_forward_xyz, its _begin / _end / _dev / _pbc variants, molecules of at most 64
 * atoms (32 where the in-kernel front-end is not used: periodic cells), update MLPs of at most [64, 64].  A molecule that would
 * take the tiled kernels, the dense and layer-level entries, the training step and the charge gradients fail with a message that says
 * so; the weight entries work as ever.  With nx <= 10 the handle is epnn_create's. */
int epnn_create_fused(const epnn_config *cfg, int device, epnn_handle **out);
int epnn_destroy(epnn_handle *h);
/* WHERE A HANDLE'S STREAM RUNS.  Every handle owns one HIP stream, and handles used side by side (engine.Pipeline: a batch in
 * flight per handle) only overlap on the GPU when their streams sit on different hardware queues: kernels of streams that share a
 * queue serialise.  The HIP runtime keeps one pool of at most GPU_MAX_HW_QUEUES hardware queues (its default: 4) per stream
 * PRIORITY CLASS -- normal, high, low -- so epnn_create places the stream by the process's count of live handle streams per
 * device and class (the placeholders of epnn_skip_hw_queues count as normal ones; epnn_destroy and epnn_skip_hw_queues(device, 0)
 * give their places back): with Q = the integer in GPU_MAX_HW_QUEUES (4 if unset or unparsable, at least 1) the classes are tried
 * in the order normal, high, low and the first with fewer than Q live streams is taken; when all are full, the one with the fewest
 * (normal first on a tie).  High / low are the `greatest` / `least` of hipDeviceGetStreamPriorityRange and exist only where they
 * differ from the default priority; a device with one level keeps every stream normal.  With Q = 4 eight handles become 4 normal
 * + 4 high, fourteen 4 + 4 + 4 and two that share; a process whose Q exceeds its handles and placeholders (this library's Python
 * binding asks for 16 when the variable is unset) sees no change at all.  Never more than 3 Q queues per process.
 * THE NULL STREAM'S PLACE.  A process that uses its null stream -- hipMemcpy, hipMemset, a kernel launched without a stream,
 * PyTorch's default stream -- has a normal hardware queue held by that stream from its first use on (measured:
 * four normal lanes then share three queues).  This library never uses it: every copy and launch of its own runs on a handle's
 * stream.  A caller whose process does says so BEFORE it creates its first handle on the device, with epnn_reserve_null_stream
 * (device, 1) or EPNN_NULL_STREAM_PLACE=1 in the environment: one place of the normal class is then left to the null stream and
 * eight handles become 3 normal + 4 high + 1 low, fourteen 3 + 4 + 4 and three that share.
 * What a caller can see of it: lanes of different classes are served in priority order, so the order in which handles used side
 * by side FINISH may differ from the order of the calls (engine.Pipeline.map collects in call order regardless); results do not
 * change by a bit.  A stream's priority is the priority of its hardware queue, and the GPU's scheduler orders the queues of ALL
 * processes on the device by it: a process that shares its GPU with other jobs takes precedence over their normal-priority work
 * with its high lanes and yields to it with its low ones -- set EPNN_STREAM_CLASSES=0 there.  The side stream of a lone handle
 * (33..64-atom molecules) stays normal and uncounted.
 * Switch: the environment variable EPNN_STREAM_CLASSES, read when a handle is created; 0 = every stream normal, as before this
 * placement existed; anything else, or unset, = on. */
/* cls: 0 normal, 1 high, 2 low -- the class epnn_create chose; priority: what hipStreamGetPriority reports for the handle's stream. */
int epnn_stream_class(epnn_handle *h, int *cls, int *priority);
/* The rule above as a pure function (no GPU needed): live[c] = live streams of the c-th class in the order tried, of which
 * the first `nclasses` (1..3) exist; limit = Q.  Returns the index of the class the next stream goes to. */
int epnn_pick_stream_class(const int live[3], int limit, int nclasses);
/* on = 1: this process uses the null stream of `device`, keep one place of the normal class for it (see above); on = 0: it does
 * not (the default; overrides EPNN_NULL_STREAM_PLACE=1, which is read when a handle is created on a device this was never called
 * for).  Makes no HIP call and may come before anything else.  It decides about the handles created afterwards: streams that
 * exist stay where they are, so call it before the first epnn_create on that device. */
int epnn_reserve_null_stream(int device, int on);
/* Leaves out `n` of the process's hardware queues: the HIP runtime deals a process's streams onto the hardware queues of their
 * priority class in the order they are created, and a pipeline of several handles runs faster with its lanes on every other
 * queue while there are twice as many queues as lanes (engine.Pipeline calls this between two handles; no counterpart in the
 * reference, which runs one model call at a time).  The placeholders are normal-priority streams and hold places of that class. */
int epnn_skip_hw_queues(int device, int n);

/* model.load_weights / layer.set_weights (infer.py:57): one Dense layer of one MLP.
 * which = EPNN_W_MSG (message_fns[t], charge_gn.py:52), EPNN_W_UPD (update_fn, t ignored, charge_gn.py:371),
 * EPNN_W_PAS (pass_fns[t], charge_gn.py:84); layer = 0..2 (EPNN_W_UPD: 0..n_hidden after epnn_set_update_layers); kernel is Keras
 * layout [in][out]. */
int epnn_set_weights(epnn_handle *h, int which, int t, int layer, const float *kernel, const float *bias);
/* model.trainable_variables / save_weights (charge_gn.py:462). */
int epnn_get_weights(epnn_handle *h, int which, int t, int layer, float *kernel, float *bias);
int epnn_weight_shape(epnn_handle *h, int which, int t, int layer, int32_t *n_in, int32_t *n_out);
/* make_model(layers, ...) / GNN_layer(message_fn, update_fn = MLP_layer(layers, out_dim = h_dim), T) (charge_gn.py:369-371): the
 * hidden widths of the update MLP, widths[n_hidden].  The default is {32, 32}.  Afterwards EPNN_W_UPD has n_hidden + 1 layers
 * (layer 0: h_dim + 32 -> widths[0]; the last: widths[n_hidden - 1] -> h_dim), all zero until epnn_set_weights fills them.
 * Fails on a handle that already holds training state (call it before epnn_train_init). */
int epnn_set_update_layers(epnn_handle *h, int n_hidden, const int32_t *widths);

/* get_init_edges (charge_gn.py:122-163): xyz[n][3] float32 -> e[n][n][e_dim] float32, host pointers. */
int epnn_edges(epnn_handle *h, int n, const float *xyz, float *e_out);
/* The same with the reference function's own parameters: num channels (charge_gn.py:122; mu = linspace(0.1, cutoff, num)),
 * cutoff and eta (the constants 3.0 and 2.0 of charge_gn.py:148-161), and, when c_out is not NULL, the cutoff weights
 * C[n][n] (float64) that get_init_edges returns tiled over the channels (charge_gn.py:163). */
int epnn_edges_ex(epnn_handle *h, int n, const float *xyz, int num, double cutoff, double eta, float *e_out, double *c_out);

/* Compact entry == gen_padded_init_state featurisation (charge_gn.py:292-366) + model([h,e,x,q,mask])
 * (charge_gn.py:369-391, infer.py:32-35) without materialising the dense (N,N,.) tensors:
 * xyz[A][3], x[A][nx] (Z + one-hot), Q[B] total charges -> q_out[A] predicted charges of the real atoms
 * (padded atoms are 0 in the reference output and are not stored).  Host pointers. */
int epnn_forward_xyz(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x,
                     const float *Q, float *q_out);
/* The same call in two halves (the loop of infer.py:62-76 with several batches in flight): _begin copies the host arrays
 * into page-locked staging owned by the handle (the caller may reuse them at once), queues uploads, kernels and the
 * download of the charges, and returns without waiting for the GPU; _end waits and writes q_out[A].  One forward per
 * handle between _begin and _end; use several handles to overlap batches (epnn_amd.engine.Pipeline.map).
 * Memory: offsets, xyz, x and Q are read before _begin returns and never afterwards, a pair-list regrow inside _end included (it
 * runs again from the staged copy); q_out is written by _end only.
 * Other entries on the SAME handle between _begin and _end (tests/test_gpu_pipeline_contract.py):
 *   refused by name, the begun forward untouched: epnn_forward_xyz_begin, epnn_forward_xyz_pbc, epnn_forward_xyz_cell (and
 *     epnn_forward_xyz, which is _begin + _end);
 *   served, with the outputs the same call gives on a fresh handle: epnn_forward_xyz_dev (and _pbc_dev / _cell_dev), the dense
 *     entries (epnn_model_forward_dense ...), epnn_charges_vjp_xyz, epnn_charges_jvp_xyz, epnn_coulomb_xyz, epnn_train_step_xyz,
 *     epnn_set_weights, epnn_set_option, epnn_sync.  Each of them first finishes what the begun forward still owes (the wait for a
 *     forward of tiled molecules and its pair-list regrow), so _end returns the charges of the begun batch, computed with the
 *     weights and options that held at _begin: new weights or options count from the next forward on. */
int epnn_forward_xyz_begin(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x,
                           const float *Q);
int epnn_forward_xyz_end(epnn_handle *h, float *q_out);
/* One large system on several GPUs (one process each, same inputs everywhere): the all-pairs sum of GNN_layer
 * (charge_gn.py:70), which is all of the cost of a system with thousands of atoms, is split by rows of atoms.  After every
 * GNN step the library calls `exchange(ctx, d_rows, row_len, n_rows, row_lo, row_hi)`: d_rows is a device array
 * [n_rows][row_len] float of which this process has filled rows row_lo..row_hi-1; the function must fill in the rows the
 * other processes own (an all-gather; epnn_memcpy_d2h / epnn_memcpy_h2d move rows) and return 0.  Molecules of at most 32
 * atoms are not partitioned.  Results are bit-identical to the unpartitioned run.
 * With exchange == NULL the handle's RCCL communicator (epnn_comm_init, same world size and rank) does it: every process
 * broadcasts its own rows in place, all of them grouped into one RCCL operation on the handle's stream -- no host
 * synchronisation inside the forward (one GPU per process; this is the multi-GPU form, the callback is the portable one). */
typedef int (*epnn_exchange_fn)(void *ctx, float *d_rows, int row_len, int n_rows, int row_lo, int row_hi);
int epnn_set_partition(epnn_handle *h, int rank, int world, epnn_exchange_fn exchange, void *ctx);
/* Same with device-resident xyz/x/Q/q_out (offsets stay on the host); asynchronous. */
int epnn_forward_xyz_dev(epnn_handle *h, int B, int N, const int32_t *offsets, const float *d_xyz,
                         const float *d_x, const float *d_Q, float *d_q_out);

/* Literal make_model call (charge_gn.py:376-389): h_inp/e_inp [B][N][N][h_dim], x_inp [B][N][N][nx],
 * q_inp/mask_inp [B][N][N][1] -> q_out [B][N][1].  Host pointers. */
int epnn_model_forward_dense(epnn_handle *h, int B, int N, const float *h_inp, const float *e_inp,
                             const float *x_inp, const float *q_inp, const float *mask_inp, float *q_out);
int epnn_model_forward_dense_dev(epnn_handle *h, int B, int N, const float *d_h_inp, const float *d_e_inp,
                                 const float *d_x_inp, const float *d_q_inp, const float *d_mask_inp,
                                 float *d_q_out);
/* GNN_layer.call (charge_gn.py:57-75): h[B][N][h_dim], e[B][N][N][e_dim], x[B][N][nx], q[B][N][1],
 * mask[B][N][N][1] -> h_out[B][N][h_dim].  Host pointers. */
int epnn_gnn_forward(epnn_handle *h, int B, int N, const float *hin, const float *e, const float *x,
                     const float *q, const float *mask, float *h_out);
/* EPN_layer.call (charge_gn.py:88-119): same inputs -> q_out[B][N][1].  Host pointers. */
int epnn_epn_forward(epnn_handle *h, int B, int N, const float *hin, const float *e, const float *x,
                     const float *q, const float *mask, float *q_out);

/* MLP_layer(nodes, out_dim, activation).call (charge_gn.py:31-45) for ANY `nodes`: n_layers Dense layers, dims[n_layers + 1] = n_in,
 * nodes..., out_dim (each 1..256), W[l] in Keras layout [dims[l]][dims[l + 1]], b[l][dims[l + 1]].  `activation` follows every layer
 * but the last (charge_gn.py:38-39: Dense(n, activation=activation) ..., Dense(out_dim, activation=None)): 0 = 'relu' (the
 * reference's default and only use), 1 = None / 'linear', 2 = 'tanh', 3 = 'sigmoid' (Keras' definitions); anything else fails.
 * x[rows][dims[0]] -> out[rows][dims[n_layers]].  Host pointers. */
int epnn_mlp_forward_layers(epnn_handle *h, int rows, int n_layers, const int32_t *dims, const float *const *W,
                            const float *const *b, const float *x, float *out, int activation);
/* MLP_layer.call (charge_gn.py:41-45) as a stand-alone operator: x[rows][n_in] -> relu 32 -> relu 32 -> out[rows][n_out];
 * kernels in Keras layout [in][out].  Host pointers. */
int epnn_mlp_forward(epnn_handle *h, int rows, int n_in, int n_out, const float *W1, const float *b1,
                     const float *W2, const float *b2, const float *W3, const float *b3, const float *x, float *out);

/* ---- training (charge_gn.py:393-402, 419): master weights, gradients and Adam moments live on the device as flat
 * vectors in model.trainable_variables order (update MLP, message MLPs t=0.., pass MLPs t=0..; kernel then bias).
 * epnn_train_init copies the current weights to the device and zeroes the Adam state (Keras-2 defaults are
 * lr 1e-3, beta1 0.9, beta2 0.999, eps 1e-7). */
int epnn_train_init(epnn_handle *h, float lr, float beta1, float beta2, float eps);
int epnn_param_count(epnn_handle *h, int64_t *out);
/* train_step on the literal make_model inputs (B,N,N,.), y and pred_out (B,N,1): loss = sum (y-p)^2, gradient of the
 * summed loss; apply != 0: all-reduce the gradient over the attached communicator (if any) and take one Adam step. */
int epnn_train_step_dense(epnn_handle *h, int B, int N, const float *h_inp, const float *e_inp, const float *x_inp,
                          const float *q_inp, const float *mask_inp, const float *y, float *pred_out, float *loss_out,
                          int apply);
/* same from a flat coordinate batch (y_flat, q_out_flat per real atom) */
int epnn_train_step_xyz(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x,
                        const float *Q, const float *y_flat, float *q_out_flat, float *loss_out, int apply);
int epnn_get_gradients(epnn_handle *h, float *out, int64_t count);
int epnn_set_gradients(epnn_handle *h, const float *in, int64_t count);
int epnn_train_apply(epnn_handle *h);
/* Charge gradients with respect to the coordinates (forces of a potential whose energy depends on the charges): for the flat
 * batch epnn_forward_xyz takes and a cotangent g[A] (one value per real atom), q_out[A] = the charges and
 * gxyz_out[A][3] = sum_i g[i] dq_i/dxyz, molecule by molecule.  N enters as in the forward (padded partners contribute to the
 * message sums); the pair and node masks are constants (they come from comparisons); the cutoff factor is smooth at the cutoff.
 * The handle's cutoff, eta and Gaussian centres are used, as in the forward.  Contract:
 *   - works on a handle that never called epnn_train_init;
 *   - uses the handle's current weights, the ones epnn_forward_xyz would use (including weights a training loop has just updated);
 *   - leaves weights, gradients (epnn_get_gradients), Adam moments and the step count untouched;
 *   - waits first for a "train_async" step still in flight;
 *   - every shape and update `layers` epnn_train_step_xyz takes: the row-fused kernels up to N = 96 ("train_fused"), the
 *     layer-by-layer ones above that and for update layers other than [32, 32];
 *   - fails (epnn_last_error) on a bad offsets array, a molecule that does not fit N, a null pointer, or two coincident atoms.
 * Bit-reproducible; a molecule's rows do not depend on the rest of the batch (at the same N).
 * Two implementations stand behind this entry and its _pbc / _cell forms (option "grad_path"): the dense path -- the training
 * step's forward + backward on rows padded to [B][N][N], whose scratch grows with B N^2 (gE alone is B N^2 48 floats) -- and the
 * pair-list path, which keeps per-atom rows and the list of pairs under the cutoff only (about 3 KB per atom and 1.1 KB per
 * listed pair; a 100 000-atom cell: 0.94 GB and 4.2 s, ten forwards: profiles/r09_grad_large.txt).  Both compute the same function (float32 rounding and
 * ReLU decisions within it apart) under the same contract; the pair-list path is built for update layers [32, 32] on a handle
 * without epnn_set_partition.  The handle keeps the scratch of its largest call on either path until epnn_destroy.  After a
 * call on the pair-list path epnn_last_stats gives out[0] = listed pairs, out[1] = 0,
 * out[2] = bytes of device scratch the call used: the checkpoints of every step (h_t, S_t, q_t), the per-atom rows and partial
 * sums of one step, the pair list and the per-pair slots; with A atoms, T steps and `pieces` = the most pieces of a molecule's
 * partner range (1 up to 32768 atoms),
 *     bytes = A (1324 + 4 nx + 324 T + 257 pieces) + 1120 listed pairs + 13 KB      (+- 256 per buffer of rounding)
 * on a handle whose first pair-list call this is (the staged inputs count with their buffer's capacity). */
int epnn_charges_vjp_xyz(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                         const float *g, float *q_out, float *gxyz_out);

/* ---- periodic systems (orthorhombic cells).  The model sees the geometry only through the pair distances D_ij of
 * get_init_edges (charge_gn.py:122-163); a periodic call replaces them by minimum-image distances and changes nothing else.
 *   box[b][0..2] (float32, Angstrom, host memory) is the cell of molecule b of the batch:
 *     box[b][k] > 0   axis k is periodic with that length, which must be at least 2 * cutoff (6 A at the default cutoff);
 *     box[b][k] == 0  axis k is open (slabs, wires; open molecules can share a batch with periodic cells);
 *     negative, NaN and infinite lengths are refused, and so is a periodic length below 2 * cutoff.
 *   Distance: per axis d = (double)x_j - (double)x_i; on a periodic axis d - k L with k = rint(d / L) (|d - k L| <= L / 2) and L
 *     the float32 length as double; D = sqrt((dx*dx + dy*dy) + dz*dz) in the order of the open case.  With L >= 2 cutoff at most
 *     one image of a pair is within the cutoff, so one e_ij per pair stays exact; where k is ambiguous (|d| near L / 2) every image
 *     is at least a cutoff away.  Coordinates need not lie in the cell.
 *   Unchanged: N and the padded partners, Q (the charge of the cell), C[D <= 0] = 1, the is_near tolerance, charge conservation.
 *   Derivative: that of a minimum-image displacement with respect to x_i / x_j is that of the unwrapped one (the image shift is
 *     constant).  Triclinic cells, and the derivative with respect to the cell (dq/dL, virial, stress), are the _cell entries below.
 *   Routing: a periodic forward always builds its pair list with the separate front-end launches; molecules of up to 32 atoms run
 *     the fused kernel on that list, larger ones the tiled kernels (the path wave_front = 0 (include/epnn_dev.h) takes).  With every box row 0 the
 *     result is bit-identical to epnn_forward_xyz with wave_front = 0 (include/epnn_dev.h), and epnn_charges_vjp_xyz_pbc to epnn_charges_vjp_xyz.
 *   A partitioned handle (epnn_set_partition) runs periodic systems too. */
int epnn_forward_xyz_pbc(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                         const float *box, float *q_out);
/* Device-resident xyz/x/Q/q_out, box rows on the host (uploaded with the call; they may change on every call, as in an NPT run). */
int epnn_forward_xyz_pbc_dev(epnn_handle *h, int B, int N, const int32_t *offsets, const float *d_xyz, const float *d_x,
                             const float *d_Q, const float *box, float *d_q_out);
/* epnn_charges_vjp_xyz in periodic cells, with its contract; coincident periodic images of two atoms are refused. */
int epnn_charges_vjp_xyz_pbc(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x,
                             const float *Q, const float *box, const float *g, float *q_out, float *gxyz_out);
/* epnn_edges_ex in the periodic cell box[3]: minimum-image edge features and cutoff weights of one system. */
int epnn_edges_pbc(epnn_handle *h, int n, const float *xyz, const float *box, int num, double cutoff, double eta, float *e_out,
                   double *c_out);
/* ---- periodic systems, general (triclinic) cells, and the strain derivative of the charges.
 *   cell[b][k][0..2] (float32, Angstrom, host memory): row k of molecule b is the lattice vector a_k.
 *     A row of three zeros is an open axis (slabs, wires; with all three rows zero an open molecule in the same batch).
 *     Refused, epnn_last_error naming molecule and axis: a NaN or infinite entry; non-zero rows that are linearly dependent; a
 *     periodic axis whose PERPENDICULAR WIDTH is below 2 * cutoff.  The width of periodic axis k is w_k = 1 / |g_k| with g_k the
 *     dual vector of a_k inside the span of the periodic rows (g_k . a_l = delta_kl for periodic l).  Three periodic rows: g_k are
 *     the columns of the inverse cell matrix, w_k = |det| / |a_l x a_m|; two: w_a = |a x b| / |b|; one: |a|.  Edge lengths do not
 *     decide it: the cell (6.5,0,0), (5,6.5,0), (0,0,7) has every edge above 6 A and a width of 5.15 A, and is refused at the
 *     default cutoff.  For a hexagonal cell with a 120 (or 60) degree angle the width is a sqrt(3) / 2: a >= 6.93 A.
 *   Distance, all in float64 from the float32 inputs: d = r_j - r_i; n_k = rint(g_k . d) for every periodic k, the dot product
 *     summed as (g_k0 dx + g_k1 dy) + g_k2 dz; d' = ((d - n_0 a_0) - n_1 a_1) - n_2 a_2 per component (each n_k a_kc is exact);
 *     D = sqrt((dx'^2 + dy'^2) + dz'^2) in the order of the open and orthorhombic code.  g_k is computed by the library on the host
 *     in float64 (cross products divided by the determinant; two rows: (b x n) / |n|^2 and (n x a) / |n|^2 with n = a x b; one
 *     row: a / |a|^2).
 *   Why that is enough: a displacement shorter than the cutoff has |g_k . d'| <= |d'| / w_k < 1/2 on every periodic axis, so with
 *     w_k >= 2 * cutoff it is the image the rounding returns, and the only image within the cutoff.  Beyond the cutoff the image
 *     returned need not be the shortest one (in a sheared cell it often is not): that does not matter, because e, C and the
 *     is_near weight are zero there -- epnn_edges_cell's C output included.  Coordinates need not lie in the cell; the cell may
 *     change on every call.
 *   Unchanged, as for box: N and the padded partners, Q (the charge of the cell), C[D <= 0] = 1, the is_near tolerance, charge
 *     conservation.  A diagonal cell diag(Lx, Ly, Lz) (zeros allowed) gives the bits of the box = (Lx, Ly, Lz) entries, an
 *     all-zero cell those of the open entries on the same route (the rule reduces to d - L rint(d / L) except at rounding ties,
 *     which lie at least a cutoff away); these entries run their own kernels for every cell, diagonal or not.
 *   Routing and the other terms of the contract are those of the _pbc twin of each entry: the separate front-end, the fused kernel
 *     on its list up to 32 atoms, the tiled kernels above; a partitioned handle works; the _dev form uploads the cell with the call
 *     and treats a changed cell as a different forward; the gradient entry leaves the training state alone and refuses
 *     coincident atoms or images.
 *   Strain derivative (gstrain_out [B][3][3], or NULL): with F = sum_i g_i q_i of one molecule and the homogeneous deformation
 *     r -> (1 + eps) r, a_k -> (1 + eps) a_k,
 *         gstrain[b][a][c] = dF/d eps_ac at eps = 0 = sum over pairs i < j with D < cutoff of (dF/dD_ij) d'_a d'_c / D_ij,
 *     accumulated in float64 per atom and summed per molecule in a fixed order (no atomics: bit-reproducible, independent of the
 *     rest of the batch), stored as the full symmetric matrix in float32.  For an open molecule pass an all-zero cell.
 *     What a caller gets from it, W = gstrain[b], H the cell matrix (rows a_k), G = inverse of H:
 *       - derivative with respect to the lattice vectors at fixed fractional coordinates:  dF/dH = G^T W   (dF/dH[k][c] = dF/da_kc);
 *       - orthorhombic cell:  dF/dL_k = W_kk / L_k;
 *       - with g = dE/dq of a potential E(q, r), W is the charges' part of the virial of E (the stress is W / volume, with the
 *         sign convention of dE/d eps); the part of E at fixed q is the caller's.
 *     gstrain_out = NULL gives the same q_out and gxyz_out bits. */
int epnn_forward_xyz_cell(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                          const float *cell, float *q_out);
/* Device-resident xyz/x/Q/q_out, cells [B][3][3] on the host (validated and uploaded with the call; they may change on every call). */
int epnn_forward_xyz_cell_dev(epnn_handle *h, int B, int N, const int32_t *offsets, const float *d_xyz, const float *d_x,
                              const float *d_Q, const float *cell, float *d_q_out);
/* epnn_edges_ex in the general cell cell[3][3]. */
int epnn_edges_cell(epnn_handle *h, int n, const float *xyz, const float *cell, int num, double cutoff, double eta, float *e_out,
                    double *c_out);
/* epnn_charges_vjp_xyz in general cells, with its contract, and the strain derivative described above. */
int epnn_charges_vjp_xyz_cell(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x,
                              const float *Q, const float *cell, const float *g, float *q_out, float *gxyz_out, float *gstrain_out);
/* ---- forward mode: the charges and their directional derivative (the other half of epnn_charges_vjp_xyz_cell, which gives
 * g^T dq/dxyz and gstrain).  For the flat batch of epnn_forward_xyz_cell, a tangent vxyz[A][3] of the coordinates, a strain tangent
 * vstrain[B][3][3] = E and a tangent vQ[B] of the total charges (each may be NULL = 0; all three NULL gives tq = 0),
 *     q_out[i]  = the charges,
 *     tq_out[i] = sum_k (dq_i/dr_k) . v_k + sum_ac (dq_i/d eps_ac) E_ac + (dq_i/dQ) vQ,     molecule by molecule:
 * the charge flux dq/dt = J v along an MD velocity (the sum_i r_i dq_i/dt part of a dipole derivative), the response of the charges
 * to a cell deformation, and with vQ = 1 alone the condensed Fukui function dq/dQ (sum_i tq_i = vQ per molecule by construction).
 * The strain is the one gstrain is defined for: r -> (1 + eps) r, a_k -> (1 + eps) a_k; image shifts, pair and node masks and the
 * is_near weights (charge_gn.py:90-94) are constants, as in the VJP.  cell [B][3][3] has the meaning and the checks of
 * epnn_forward_xyz_cell (a diagonal cell is a box, a zero row an open axis); NULL: open molecules.
 *   Edges (get_init_edges, charge_gn.py:122-163): for a listed pair with the front-end's image d' and distance D, in float64,
 *     tD = d' . (v_j - v_i) / D + d'^T E d' / D,     te_k = (C'(D) - 2 eta (D - mu_k) C(D)) exp(-eta (D - mu_k)^2) tD,
 *   stored as a float32 row te[P][48].
 *   GNN_layer.call (charge_gn.py:57-75), per step in the factorised form: ta_i = [0 | th_i | vQ / n], tP = Wi^T ta, tR = Wj^T ta;
 *     z1 = relu(P_i + R_j + We^T e_ij), tz1 = [z1 > 0] (tP_i + tR_j + We^T te_ij); z2 = relu(W2^T z1 + b2), tz2 = [z2 > 0] W2^T tz1;
 *     tS_i = sum over all N partners of tz2 (an all-pairs sweep on f32 MFMA tiles for the pairs without e, the listed pairs as
 *     corrections, the (N - n) padded partners in closed form); tM = W3^T tS; th' = the update MLP's tangent on [th | tM].
 *   EPN_layer.call (charge_gn.py:88-119), per step: tq_i += sum over listed j of w_ij (tf_ij - tf_ji) / 2 with tf the tangent of the
 *     pass MLP on [a_i | a_j | e_ij], a = [x | h_T | q_t], ta = [0 | th_T | tq_t].
 * Contract: that of the pair-list path of epnn_charges_vjp_xyz ("grad_path" = 2), whatever that option is set to: works on a handle
 * that never trained, uses the current weights, leaves weights, gradients, Adam state and step count untouched, waits first for a
 * "train_async" step in flight; refuses by name update layers other than [32, 32], a partitioned handle, bad offsets, a molecule
 * that does not fit N, null xyz / x / Q / outputs, coincident atoms or images (the handle stays usable); h_dim below 48 runs
 * zero-padded; bit-reproducible (no float atomics, every sum in a fixed order); a molecule's rows do not depend on the rest of the
 * batch at the same N.  q_out has the bits of that path's q_out: the primal is its checkpointed forward, operation by operation,
 * and every ReLU decision of a tangent is taken from the float32 pre-activation its backward takes it from, so that
 * sum_i g_i tq_i = gxyz . v + gstrain : E holds between the two entries to float32 rounding of the sums.
 * One call costs about one extra forward of that path, keeps no checkpoints and nothing of size N^2.  Device scratch, with
 * pieces = max over the molecules of min(16, ceil(2048 / ceil(n / 16))):
 *     bytes = A (1592 + 4 nx + 257 pieces) + 980 listed pairs + 13 KB      (12 A more with vxyz; +- 256 per buffer of rounding)
 * shared with the gradient path: the handle keeps the scratch of its largest call of either until epnn_destroy.  After a call
 * epnn_last_stats gives out[0] = listed pairs, out[1] = 0, out[2] = bytes of device scratch the call used. */
int epnn_charges_jvp_xyz_cell(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                              const float *cell, const float *vxyz, const float *vstrain, const float *vQ, float *q_out,
                              float *tq_out);
/* ---- forward mode, K directions in one pass: epnn_charges_jvp_xyz_cell with K tangents beside one primal.  K is in 1..16 (any
 * other value is refused by name; the handle stays usable).  vxyz[K][A][3], vstrain[K][B][3][3], vQ[K][B]: each may be NULL (= 0 for
 * every tangent; all three NULL gives tq = 0).  q_out[A] is computed once; tq_out[K][A]: row k has exactly the definition of
 * epnn_charges_jvp_xyz_cell's tq_out for the k-th slices -- six unit strains give the full strain response dq_i/d eps_ab in one call,
 * three Cartesian directions (or one per normal mode) a dipole derivative, 3 n directions a forward-mode Jacobian of a molecule.
 * Contract: that of epnn_charges_jvp_xyz_cell, word for word: the pair-list path whatever "grad_path" says; works on a handle that
 * never trained, uses the current weights, leaves weights, gradients, Adam state and step count untouched, waits first for a
 * "train_async" step in flight; refuses by name update layers other than [32, 32], a partitioned handle, bad offsets, a molecule
 * that does not fit N, null xyz / x / Q / outputs, coincident atoms or images (the handle stays usable); h_dim below 48 runs
 * zero-padded; no float atomics and every sum in a fixed order; a molecule's rows do not depend on the rest of the batch at the
 * same N.
 * Bits: q_out has the bits of epnn_charges_jvp_xyz_cell (and so of the pair-list gradient path), and row k of tq_out the bits that
 * entry gives for tangent k alone: that entry is K = 1 of this one, and no tangent statement reads another tangent (the same MFMA
 * order per tangent, the same pieces, slot order and closed-form padded term).  A row therefore does not depend on K, on its
 * position, or on what the other rows hold.
 * Cost: the front-end, the pair list, the primal projections, pair and atom kernels run once; the all-pairs sweep carries the
 * tangents in chunks of 4, 2 or 1 (the widest that fits what is left: K = 7 is 4 + 2 + 1) and each chunk's launch repeats the 16
 * primal MFMAs per partner for its masks: sum over chunks of (16 + 16 kc) MFMAs per partner and tile against 32 K for K single
 * calls; measured, a K = 4 call on a 10 000-atom cell takes 0.68 of four single calls, while on batches of small molecules K single
 * calls are faster from K = 4 on (profiles/r12_jvp_multi.txt).  Device scratch: the tangent rows (te, th, tP, tR, the sweep's
 * tangent pieces, the tangent slots, tq) are K times the single call's, the primal rows and the pair list are not multiplied:
 *     bytes = A (940 + 4 nx + 129 pieces + K (652 + 128 pieces)) + (524 + 456 K) listed pairs + 13 KB
 *                                                              (12 K A more with vxyz; +- 256 per buffer of rounding)
 * which at K = 1 is epnn_charges_jvp_xyz_cell's formula.  Shared with the gradient and single-tangent calls: the handle keeps the
 * scratch of its largest call.  After a call epnn_last_stats gives out[0] = listed pairs, out[1] = 0, out[2] = bytes of device
 * scratch the call used. */
int epnn_charges_jvp_multi_xyz_cell(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                                    const float *cell, int K, const float *vxyz, const float *vstrain, const float *vQ, float *q_out,
                                    float *tq_out);
/* ---- reverse mode, K cotangents in one pass: epnn_charges_vjp_xyz_cell with K seeds beside one primal.  K is in 1..16 (any other
 * value is refused by name; the handle stays usable).  g[K][A]: the cotangents.  q_out[A] is computed once; gxyz_out[K][A][3] and
 * gstrain_out[K][B][3][3] (or NULL): row k is, word for word, gxyz_out / gstrain_out of epnn_charges_vjp_xyz_cell on "grad_path" 2
 * called with g[k].  cell [B][3][3] has the meaning and the checks of epnn_charges_vjp_xyz_cell; NULL: open molecules.  Three seeds
 * g = x, y, z (coordinates relative to a fixed origin) give the charge-flux part of the atomic polar tensor,
 *     d mu_a / d r_ib = q_i delta_ab + sum_k r_ka dq_k/dr_ib,        mu = sum_k q_k r_k,
 * in one call (engine.py dipole_xyz); K potentials give K force sets.
 * Contract: that of the pair-list path of epnn_charges_vjp_xyz: the entry always runs from the pair list, whatever "grad_path"
 * says; works on a handle that never trained, uses the current weights, leaves weights, gradients, Adam state and step count
 * untouched, waits first for a "train_async" step in flight and finishes a forward begun with epnn_forward_xyz_begin, as the single
 * entry does; refuses by name update layers other than [32, 32], a partitioned handle, a fused-only handle, bad offsets, a molecule
 * that does not fit N, a null required pointer, coincident atoms or images (the handle stays usable); h_dim below 48 runs
 * zero-padded; no float atomics and every sum in a fixed order; a molecule's rows do not depend on the rest of the batch at the
 * same N.
 * Bits: q_out has the bits of epnn_charges_vjp_xyz_cell on "grad_path" 2, and row k the bits that entry gives for g[k] alone,
 * whatever K, the row's position and the other rows are; gstrain_out = NULL changes no other bit.  No cotangent statement reads
 * another cotangent, and the single entry runs these kernels at K = 1: one fmaf chain or MFMA sequence per cotangent, accumulators
 * from zero, the same pieces and slot order.
 * Cost: the front-end, the pair list, the checkpointed forward, the primal projections and every pair's and atom's primal
 * pre-activations and masks run once; the two all-pairs backward sweeps carry the cotangents in chunks of 4, 2 or 1 (K = 7 is
 * 4 + 2 + 1) and each chunk's launch repeats the 16 primal MFMAs per partner: sum over chunks of 2 (16 + 16 kc) MFMAs per partner and
 * tile against 64 K for K single calls (profiles/r24_vjp_multi.txt).  Device scratch: the single entry's inputs, pair list,
 * checkpoints and primal rows once and K copies of the cotangent rows gq, gh, ghp, dS, the sweeps' pieces, the slots, gE, the
 * coordinate slots, the strain shares and the outputs; with `pieces` as at epnn_charges_vjp_xyz,
 *     bytes = A (744 + 4 nx + 324 T + pieces + K (580 + 256 pieces)) + (268 + 848 K) listed pairs + 36 K B + 13 KB
 *                                                                                         (+- 256 per buffer of rounding)
 * which at K = 1 is epnn_charges_vjp_xyz's formula, with the staged inputs counted by this call's bytes.  Shared with the other pair-list calls: the handle keeps the scratch of its
 * largest call.  After a call epnn_last_stats gives out[0] = listed pairs, out[1] = 0, out[2] = bytes of device scratch the call used.
 * Out of scope: a dense-path twin; dF/dQ, the adjoint of the JVP's vQ; box rows (a box is its diagonal cell, whose bits are the box
 * entry's). */
int epnn_charges_vjp_multi_xyz_cell(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                                    const float *cell, int K, const float *g, float *q_out, float *gxyz_out, float *gstrain_out);
/* ---- electrostatics of the predicted charges in one call: charges, potential, Coulomb energy and total forces.  Replaces the three
 * steps of INTEGRATION.md, "Forces from the charges" (a forward, the caller's own all-pairs sum for g = dE/dq, a gradient call with
 * a second forward inside) for the potential most used with a charge model.  Per molecule b of the flat batch, over its real atoms
 * only (the N - n padded partners have no coordinates: they enter the model's message sums as in every entry, not these sums):
 *     kappa(D) = 1 / D                  alpha == 0: bare Coulomb
 *              = erf(alpha D) / D       alpha  > 0: Gaussian-smeared charges of equal width sigma, alpha = 1 / (2 sigma)
 *     phi_i    = ke sum_{j != i} q_j kappa(D_ij)                                         = dE/dq_i
 *     E_b      = 1/2 sum_i q_i phi_i                                                     = ke sum_{i<j} q_i q_j kappa(D_ij)
 *     ffix_i   = -ke q_i sum_{j != i} q_j kappa'(D_ij) (r_i - r_j) / D_ij                = -dE/dr_i at fixed q
 *     fq_i     = -sum_k phi_k dq_k/dr_i        = -gxyz_out of epnn_charges_vjp_xyz with g = phi
 *     f_i      = ffix_i + fq_i  (one float32 add per component)                          = -dE/dr_i, total
 * ke is the caller's unit constant (14.3996454784255 eV A / e^2, 332.0637 kcal A / mol e^2).  q is the model's output, so sum q = Q
 * holds by construction and no constraint term appears.  Open systems only: the entry takes no box or cell (fully periodic cells:
 * epnn_coulomb_xyz_cell below, an Ewald sum; slabs, two periodic axes: epnn_coulomb_xyz_slab below).  No self-energy term (for alpha > 0 the
 * Gaussians' self-energy -ke alpha / sqrt(pi) sum q_i^2 is left out; it depends on q alone; the entry with it, with per-atom widths and
 * with on-site terms: epnn_coulomb_xyz_site below).  Every pair of a molecule counts in full
 * here; bonded exclusions and the scaling of near neighbours: epnn_coulomb_xyz_excl below.
 * Outputs (host): q_out[A], phi_out[A], e_out[B] in float64 (a float32 energy of a 100 000-atom system loses the digits its forces
 * live in), f_out[A][3]; ffix_out[A][3] and fq_out[A][3] may each be NULL, and the other outputs have the same bits either way.
 * Contract: that of epnn_charges_jvp_xyz_cell, word for word where it applies: the pair-list path whatever "grad_path" says; works
 * on a handle that never trained, uses the current weights, leaves weights, gradients, Adam state and step count untouched, waits
 * first for a "train_async" step in flight; refuses by name update layers other than [32, 32], a partitioned handle, bad offsets,
 * a molecule that does not fit N, a null required pointer, ke not finite, alpha negative or not finite, two coincident atoms (the
 * handle stays usable); h_dim below 48 runs zero-padded; bit-reproducible (no float atomics, every sum in a fixed order); a
 * molecule's rows do not depend on the rest of the batch at the same N.
 * Bits: q_out has the bits of epnn_charges_vjp_xyz on "grad_path" 2; fq_out is bit for bit -gxyz_out of that entry called with
 * g = phi_out; f_out == ffix_out + fq_out in float32.  The call is that entry's pair-list call with one forward: set-up and
 * checkpointed forward, an all-pairs Coulomb sweep on that forward's charges which writes phi into the backward's seed on the
 * device, the backward, one download.  Pair terms are float32 (one reciprocal square root per pair; erff, and expf or a series,
 * for alpha > 0) of displacements taken in float64 and rounded once, so atoms far from the origin lose nothing; phi, ffix and E
 * accumulate in float64: each is within 2e-6 of the sum of its absolute terms, whatever n.
 * Device scratch: the gradient path's rows (the formula at epnn_charges_vjp_xyz, without the 4 A bytes of its staged g) plus what
 * the Coulomb sweep adds -- its float64 partial rows [cpieces][A][4], the atoms' energy shares, phi and ffix, E, the task table:
 *     bytes = gradient path's + A (20 + 32 cpieces) + 8 B + 16 ctasks
 * and, term by term, with the staged inputs counted with this call's bytes (not with their buffer's capacity):
 *     bytes = A (1344 + 4 nx + 324 T + 256 pieces + 32 cpieces) + 16 (gtasks + ctasks) + 1116 max(listed pairs, 1) + 56 B + 8240
 *                                                                  (plus up to 256 per buffer of rounding; 44 buffers)
 * pieces and gtasks as on the gradient path: pieces = max over the molecules of p(n) = min(16, ceil(2048 / ceil(n / 16))), gtasks =
 * sum of ceil(n / 16) p(n); cpieces = max of c(n) = 1 up to 64 atoms, else min(32, ceil(n / 128), ceil(2048 / ceil(n / 64)));
 * ctasks = one per wavefront of molecules of up to 64 atoms packed in batch order plus ceil(n / 64) c(n) per larger molecule.
 * Shared with the other pair-list calls: the handle keeps the scratch of its largest call.  After a call epnn_last_stats gives
 * out[0] = listed pairs, out[1] = 0, out[2] = bytes of device scratch the call used. */
int epnn_coulomb_xyz(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                     double ke, double alpha, float *q_out, float *phi_out, double *e_out, float *f_out,
                     float *ffix_out, float *fq_out);
/* ---- electrostatics of the predicted charges in fully periodic cells: epnn_coulomb_xyz by an Ewald sum (INTEGRATION.md,
 * "Electrostatics in one call", the periodic section).  cell [B][3][3] as in epnn_forward_xyz_cell, every axis periodic.  ke and
 * alpha as above; e_alpha(D) = 1 for alpha == 0 and erf(alpha D) for alpha > 0; beta the splitting parameter, V = |det H|,
 * Q = sum_i q_i, d_ij the minimum-image displacement and D = |d_ij|; g(u) as above with g_0 = 1:
 *     real         kappa_s(D) = [e_alpha(D) - erf(beta D)] / D for j != i and D <= rc, zero beyond; kappa_s' = -[g_alpha - g_beta] / D^2.
 *                  With rc <= w_min / 2 (w_min the smallest perpendicular width) the image found by rounding the fractional
 *                  difference is the only one in range and no atom meets an image of itself.
 *     reciprocal   k = 2 pi (m0 g_0 + m1 g_1 + m2 g_2) != 0 with |k| <= kc;  c(k) = ke (4 pi / V) exp(-k^2 / 4 beta^2) / k^2;
 *                  S(k) = sum_j q_j exp(i k r_j);  phi_i += sum_k c(k) Re[exp(-i k r_i) S(k)];  E_rec = 1/2 sum_k c(k) |S(k)|^2;
 *                  ffix_i -= q_i sum_k c(k) k Im[exp(-i k r_i) S(k)]   (= -dE_rec/dr_i; the half space is summed, doubled)
 *     self         phi_i -= ke (2 beta / sqrt(pi)) q_i          (the split's own term, there for alpha == 0 too: no beta is left)
 *     background   phi_i -= ke pi Q / V (1 / beta^2 - [alpha > 0] / alpha^2): the neutralising background of a charged cell (the
 *                  model conserves Q, which need not be 0); uniform, so it does not change fq (sum_i dq_i/dr = 0)
 *     energy       E = 1/2 sum_i q_i phi_i per cell
 *     strain at fixed charges (the convention of epnn_charges_vjp_xyz_cell's gstrain_out: homogeneous strain of coordinates and cell)
 *                  real 1/2 ke sum_{i != j} q_i q_j kappa_s'(D) d_a d_b / D;  reciprocal 1/2 sum_k c(k) |S|^2 [-delta_ab + 2 k_a k_b
 *                  (1 / k^2 + 1 / 4 beta^2)] over the whole sphere;  background -E_bg delta_ab, E_bg = -ke pi Q^2 / (2 V) (1 / beta^2 -
 *                  [alpha > 0] / alpha^2);  the self term has none.
 * epnn_ewald_params (host only, no handle, no device) holds the rule for one cell [3][3]: s = sqrt(-ln tol), rc = w_min / 2,
 * beta = s / rc, and where alpha > 0 beta = min(beta, alpha) -- at beta == alpha the real-space term vanishes identically, rc is
 * reported as 0 and the sweep is skipped; kc = 2 beta s, M_k = ceil(kc |a_k| / 2 pi).  out [6] = beta, rc, kc, M0, M1, M2.  What tol
 * means: against the same sum at tol = 1e-14, phi agrees within tol ke beta sum_j |q_j|, E within tol 1/2 ke beta (sum_j |q_j|)^2,
 * ffix within tol ke beta^2 sum_j |q_j| max_j |q_j| (measured 0.02 to 0.03 of these on a 20-atom sheared cell).  It refuses, by
 * name: a cell with an open axis (two- and one-dimensional Ewald sums are different mathematics), dependent rows, an entry that is
 * not finite, alpha negative or not finite, tol outside (0, 1), and a cell whose k box (2 M0 + 1)(2 M1 + 1)(M2 + 1) exceeds
 * 2^18 slots (extreme aspect ratios are refused, not served slowly).
 * epnn_coulomb_xyz_cell takes the numbers, ewald [B][6] (host, float64, a row per cell as epnn_ewald_params writes it), checks
 * that beta > 0, 0 <= rc <= w_min / 2 (rc == 0 only with beta == alpha > 0), that every M_k is an integer of at least
 * ceil(kc |a_k| / 2 pi) and that the k box is under the cap, and runs at exactly those values.
 * Outputs (host): q_out[A], phi_out[A], e_out[B] float64 (per cell), f_out[A][3] the total forces, gstrain_out[B][3][3] the total
 * strain derivative dE/d eps (the part at fixed charges plus the part through dq/d eps); ffix_out, fq_out, gstrain_fix_out and
 * gstrain_q_out may each be NULL and the other outputs have the same bits either way.
 * Bits: q_out, fq_out = -gxyz_out and gstrain_q_out = gstrain_out of epnn_charges_vjp_xyz_cell on "grad_path" 2 called with
 * g = phi_out; f_out == ffix_out + fq_out and gstrain_out == gstrain_fix_out + gstrain_q_out in float32.
 * Contract: that of epnn_coulomb_xyz (the pair-list path whatever "grad_path" says, no training state touched, the same refusals;
 * the cell is checked as in epnn_forward_xyz_cell), and a cell's rows do not depend on the rest of the batch at the same N.
 * Arithmetic: the real-space part is the open call's all-pairs sweep with the minimum image of each pair (float64 displacement
 * through the cell, rounded once; no cell list, no image loop); S(k) per cell and k slot and the reciprocal sums per atom take the
 * phase as 2 pi frac(m . s_j) from fractional coordinates reduced in float64, so unwrapped coordinates cost nothing.  Per-pair and
 * per-(atom, k) terms are float32, every running sum float64, no float atomics.  phi, ffix, E and the fixed-charge strain are each
 * within 2e-6 of the sum of their absolute real-space terms plus 34 * 2^-24 of the sum of their absolute reciprocal terms
 * (tests/test_gpu_coulomb_cell.py counts the roundings; measured: 0.03 of that at worst).
 * Device scratch on top of the gradient path's: A (20 + 80 cpieces + 56) + 44 B + 32 slots + the task tables and 72 B of
 * parameters; slots = the batch's k slots, about 3600 for a cube at tol = 1e-6 whatever its size.  Nothing of size n nk or n^2.
 * Still missing: one periodic axis (wires); the strain derivative of the slab sum; PME (bonded exclusions: epnn_coulomb_xyz_cell_excl
 * below; two periodic axes: epnn_coulomb_xyz_slab below).  The slab sum's strain derivative has since been built as an entry of its
 * own, epnn_coulomb_xyz_slab_strain, behind epnn_coulomb_xyz_slab; per-atom Gaussian widths, the Gaussians' self-energy and on-site
 * terms: epnn_coulomb_xyz_site and epnn_coulomb_xyz_cell_site below. */
int epnn_ewald_params(const float *cell, double alpha, double tol, double *out);
int epnn_coulomb_xyz_cell(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                          const float *cell, const double *ewald, double ke, double alpha, float *q_out, float *phi_out,
                          double *e_out, float *f_out, float *gstrain_out, float *ffix_out, float *fq_out,
                          float *gstrain_fix_out, float *gstrain_q_out);
/* ---- bonded exclusions and pair scaling for the two calls above ("Electrostatics in one call": a water box with
 * bonded_exclusions).  Every classical force field removes the 1-2 and 1-3 Coulomb terms and scales 1-4; a correction applied by
 * the caller afterwards would leave fq and the charges' part of the strain wrong, because phi is the backward's seed on the device.
 * The list: npairs unordered pairs (ex_i[p], ex_j[p]) of flat atom indices with a factor ex_scale[p] (host).  A listed pair interacts
 * with weight s_p instead of 1: 0 excludes, 0.5 or 0.8333 scales, 1 changes nothing.  With w_ij = s_p for listed pairs and 1 otherwise:
 *     open       phi_i  = ke sum_{j != i} w_ij q_j kappa(D_ij) = dE/dq_i (w is symmetric);   E_b = 1/2 sum_i q_i phi_i
 *                ffix_i = -ke q_i sum_{j != i} w_ij q_j kappa'(D_ij) (r_i - r_j) / D_ij;      fq, f as above, with this phi as the seed
 *     periodic   the Ewald sum of epnn_coulomb_xyz_cell over all pairs and images exactly as there, plus, for the one image d of each
 *                listed pair that the cell's rounding rule returns (D = |d|), with the bare kappa_alpha = e_alpha(D) / D (no beta):
 *                phi_i += ke (s - 1) q_j kappa_alpha(D);   ffix_i -= ke (s - 1) q_i q_j kappa_alpha'(D) d / D;
 *                gstrain_fix += ke (s - 1) q_i q_j kappa_alpha'(D) d_a d_b / D, once per listed pair;   E = 1/2 sum q_i phi_i.
 *                The correction is the same whatever beta, rc and kc are, and it is there when rc == 0 and the sweep is skipped.
 * Contract: that of the entry each extends, word for word, plus: npairs == 0 is allowed (the three list pointers may then be NULL)
 * and gives the bits of the plain entry on every output; so does a list whose factors are all 1 (the correction adds exact zeros to
 * float64 sums); the outputs depend neither on the order of the list nor on which atom of a pair is named first (the host sorts the
 * list into a CSR by atom: every pair in both directions, every row by partner index); a molecule's rows depend neither on the rest
 * of the batch nor on the other molecules' pairs.  Refused by name, each message with the pair's position in the list, the handle
 * stays usable: npairs < 0 or 2 npairs > 2^31 - 1; a NULL list with npairs > 0; an index outside [0, A); i == j; the two atoms in
 * different molecules; a pair listed twice, in either order; a factor that is not finite; and, in the periodic entry after the device
 * pass, a listed pair farther apart than half the smallest perpendicular width of its cell (beyond it the rounding rule no longer
 * returns the nearest image; bonded atoms are never that far apart).
 * Bits: q_out has the bits of the plain entry; fq_out and gstrain_q_out are bit for bit -gxyz_out and gstrain_out of
 * epnn_charges_vjp_xyz[_cell] on "grad_path" 2 called with g = phi_out; f = ffix + fq and gstrain = gstrain_fix + gstrain_q in float32.
 * Arithmetic: one kernel more, an atom per lane walking its CSR row in partner order; the pair term is the open sweep's float32 term
 * (float64 displacement, through the cell's minimum image in the periodic entry, rounded once; one reciprocal square root; erff and
 * g for alpha > 0) times the float32 factor s - 1, summed in float64 into one row per atom, which the atoms' kernel adds as one more
 * piece behind the sweep's.  The plain entries keep their kernels, paths, bits and scratch.
 * Accuracy: phi, ffix, E and the fixed-charge strain are each within 2e-6 of the sum of the absolute values of the terms actually
 * added: the all-pairs (or real-space) terms AND the listed pairs' correction terms |(s - 1) term| -- an excluded pair's full term is
 * added by the sweep and taken away by the correction, so both count in the yardstick -- plus 34 * 2^-24 of the absolute reciprocal
 * terms in the periodic entry.  A correction term has the sweep's roundings and one multiply by the factor, about 11 * 2^-24.
 * Device scratch (epnn_last_stats out[2]) on top of the plain entry's, with P = npairs: the staged CSR and the correction's rows,
 *     open      (A + 1) 4 + 16 P + 32 A          periodic  (A + 1) 4 + 16 P + 80 A          (two buffers: plus up to 256 of rounding each) */
int epnn_coulomb_xyz_excl(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                          double ke, double alpha, int64_t npairs, const int32_t *ex_i, const int32_t *ex_j, const float *ex_scale,
                          float *q_out, float *phi_out, double *e_out, float *f_out, float *ffix_out, float *fq_out);
int epnn_coulomb_xyz_cell_excl(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                               const float *cell, const double *ewald, double ke, double alpha, int64_t npairs, const int32_t *ex_i,
                               const int32_t *ex_j, const float *ex_scale, float *q_out, float *phi_out, double *e_out, float *f_out,
                               float *gstrain_out, float *ffix_out, float *fq_out, float *gstrain_fix_out, float *gstrain_q_out);
/* ---- per-atom Gaussian widths, self-energy and on-site terms: the energy of the potentials built on a charge model (4G-HDNNP, CENT,
 * QEq-style models driven by predicted charges; INTEGRATION.md, "Charge-model energies: widths, hardness, electronegativity"),
 *     E = sum_i (chi_i q_i + 1/2 J_i q_i^2) + ke sum_i q_i^2 / (2 sqrt(pi) sigma_i) + ke sum_{i<j} q_i q_j erf(gamma_ij D_ij) / D_ij,
 *     gamma_ij = 1 / sqrt(2 (sigma_i^2 + sigma_j^2)),
 * for open molecules and fully periodic cells (slabs: epnn_coulomb_xyz_slab_site below).  A caller cannot add these terms afterwards: phi is the backward's seed on the device,
 * and a term of dE/dq added outside leaves fq and the charges' part of the strain wrong.
 * New inputs, all host arrays, float32, one value per real atom:
 *     sigma[A]     may be NULL: every pair then uses the call's alpha, as in the entries above.  Otherwise every value is finite and
 *                  positive, 2 sigma^2 rounded to float32 is a positive finite float, and alpha must be 0 (both given is refused by
 *                  name).  Equal widths sigma are the existing alpha = 1 / (2 sigma).
 *     chi[A], hard[A] (J)   may each be NULL (= 0); in the caller's energy units per charge and per charge squared, NOT multiplied by
 *                  ke; they must be finite.
 *     self_term    0 or 1.  With 1, E_self = ke sum_i gamma_ii q_i^2 / sqrt(pi) is added, gamma_ii = 1 / (2 sigma_i), or alpha when sigma
 *                  is NULL.  self_term = 1 with neither sigma nor alpha > 0 is refused by name (a point charge's self-energy is infinite).
 *     the list     (npairs, ex_i, ex_j, ex_scale) has the meaning, the checks and the refusals of epnn_coulomb_xyz_excl / _cell_excl;
 *                  npairs == 0 with NULL pointers is allowed: one entry per geometry.  A listed pair gets (s - 1) times its bare
 *                  erf(gamma_ij D) / D term; w_ij = s for listed pairs and 1 otherwise.
 * Open:
 *     phi_i  = ke [ sum_{j != i} w_ij q_j erf(gamma_ij D_ij) / D_ij  +  [self_term] 2 gamma_ii q_i / sqrt(pi) ]
 *     mu_i   = chi_i + J_i q_i + phi_i                        = dE/dq_i, the seed of the backward
 *     E_b    = sum_i [ chi_i q_i + 1/2 J_i q_i^2 + 1/2 q_i phi_i ]                                       (float64)
 *     ffix_i = -ke q_i sum_{j != i} w_ij q_j kappa_ij'(D_ij) (r_i - r_j) / D_ij,   kappa_ij' = -g(gamma_ij D) / D^2
 *     fq_i   = -sum_k mu_k dq_k/dr_i,     f = ffix + fq     (one float32 add)
 * Fully periodic cells: the sum of epnn_coulomb_xyz_cell with gamma_ij in place of alpha in the real-space term
 * [erf(gamma_ij D) - erf(beta D)] / D, D <= rc; the point-charge reciprocal and -2 beta / sqrt(pi) q_i terms stay as they are.  The
 * background of a charged cell is worked out per pair, from int (1/D - erf(gamma D)/D) d^3D = pi / gamma^2:
 *     phi_bg_i = -ke (pi / V) [ Q / beta^2 - 2 sigma_i^2 Q - 2 sum_j q_j sigma_j^2 ]                     (j == i included)
 * which is the existing background for equal widths; the uniform constant 2 ke pi / V sum_j q_j sigma_j^2 is there for Q = 0 too.
 * E_bg = 1/2 sum_i q_i phi_bg_i, with strain -E_bg delta_ab; the real-space virial and the listed pairs' virial are the existing sums
 * with the new g; the self and on-site terms have no strain; gstrain_q = sum_k mu_k dq_k/d eps comes from the backward's strain rows.
 * The cell entry runs at the ewald [B][6] numbers it is given, as epnn_coulomb_xyz_cell does; with sigma use
 * epnn_ewald_params(cell, 0, tol).  It refuses by name a cell whose widest Gaussian does not fit the split: gamma_min = 1 / (2 sigma_max)
 * >= beta is required, and the message names the cell, sigma_max and the largest width 1 / (2 beta) allowed (beyond it the
 * erf(gamma D) tail at rc is no longer under what tol means; a larger tol or the caller's own row with a smaller beta moves the limit).
 * With sigma NULL and alpha > 0 the existing rule (beta capped at alpha, rc = 0) applies unchanged.
 * Outputs: those of the _excl entries plus mu_out[A]; mu_out, ffix_out, fq_out, gstrain_fix_out and gstrain_q_out may each be NULL
 * and the other outputs have the same bits either way.
 * Contract: that of the _excl entries, word for word: the pair-list path whatever "grad_path" says, no training state touched, waits
 * for a "train_async" step, the same refusals with the handle left usable, no float atomics, every sum in a fixed order, a molecule's
 * rows independent of the rest of the batch and of the list's order.  Refused by name besides: sigma with alpha > 0; a sigma that is
 * zero, negative or not finite, or whose 2 sigma^2 is not a positive finite float32; chi or hard not finite; self_term other than 0 or
 * 1, or 1 with neither sigma nor alpha > 0; a cell whose sigma_max exceeds 1 / (2 beta).
 * Bits: q_out has the bits of epnn_charges_vjp_xyz[_cell] on "grad_path" 2; fq_out and gstrain_q_out are bit for bit -gxyz_out and
 * gstrain_out of that entry called with g = mu_out; f == ffix + fq and gstrain == gstrain_fix + gstrain_q in float32.  With sigma, chi
 * and hard all NULL and self_term = 0 the call runs the existing kernels: every output has the bits of epnn_coulomb_xyz_excl /
 * _cell_excl on the same arguments, and mu_out == phi_out.
 * Arithmetic: the sweeps and the listed pairs' kernel take a third pair-term mode, a template parameter beside "bare" and
 * "erf(alpha)": the lane holds w_i = 2 sigma_i^2, the partners' w_j are staged beside their charges in LDS, gamma = rsqrtf(w_i + w_j)
 * per pair, then the erff / g path of alpha > 0 with gamma for alpha (one add, one reciprocal square root and one multiply more in
 * front of erff, about 4 * 2^-24 on the argument, and |u erf'(u)| <= erf(u): the bounds of the entries above hold).  One float4 per atom,
 * (2 sigma^2, chi, J, gamma_ii), is made on the host in float64, rounded once and staged as one more span; the atoms' kernels add the
 * self term to phi, write mu = chi + J q + phi into the seed and into mu_out, and q (chi + 1/2 J q) + 1/2 q phi into the energy share,
 * in float64.  The on-site terms are exact float64 products of float32 values: they add 2 * 2^-24 of |chi_i| + |J_i q_i| to mu's error,
 * its rounding to float32.  Cells: one wavefront per cell adds sum_j q_j 2 sigma_j^2 in the order of the energy sum.
 * Device scratch (epnn_last_stats out[2]) on top of the _excl entry's on the same batch and list (for npairs == 0: the plain entry's),
 * when any of sigma, chi, hard, self_term is given: the staged rows [A] float4, one buffer more (plus up to 256 of rounding), mu [A]
 * at the end of the outputs' buffer and, in cells, the per-cell sums [B] float64 at the end of the sweep's buffer (a buffer that
 * grows moves its rounding to 256 by less than 256 either way):
 *     open      16 A + 4 A          periodic  16 A + 4 A + 8 B */
int epnn_coulomb_xyz_site(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                          double ke, double alpha, const float *sigma, const float *chi, const float *hard, int self_term,
                          int64_t npairs, const int32_t *ex_i, const int32_t *ex_j, const float *ex_scale,
                          float *q_out, float *phi_out, float *mu_out, double *e_out, float *f_out, float *ffix_out, float *fq_out);
int epnn_coulomb_xyz_cell_site(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                               const float *cell, const double *ewald, double ke, double alpha, const float *sigma, const float *chi,
                               const float *hard, int self_term, int64_t npairs, const int32_t *ex_i, const int32_t *ex_j,
                               const float *ex_scale, float *q_out, float *phi_out, float *mu_out, double *e_out, float *f_out,
                               float *gstrain_out, float *ffix_out, float *fq_out, float *gstrain_fix_out, float *gstrain_q_out);
/* ---- electrostatics of the predicted charges in slab cells: epnn_coulomb_xyz for two periodic axes and one open axis (surfaces,
 * membranes, electrodes, adsorbed layers), by the exact two-dimensional Ewald sum (Parry; Heyes, Barber and Clarke; de Leeuw and
 * Perram; INTEGRATION.md, "Electrostatics in one call", the section "Slabs").  cell [B][3][3] as in epnn_forward_xyz_cell with
 * exactly one row of zeros, the open axis, at any of the three places (the distance rule: "A row of three zeros is an open axis"
 * above).  a, b the two periodic rows, A = |a x b|, nhat = (a x b) / A, g_a, g_b their dual vectors, d_ij = r_i - r_j,
 * z_ij = nhat . d_ij; ke, alpha, e_alpha and g as in epnn_coulomb_xyz_cell; beta the splitting parameter:
 *     real         kappa_s(D) = [e_alpha(D) - erf(beta D)] / D over the minimum image of every pair j != i with D <= rc, zero beyond
 *                  (rc <= w_min / 2 over the two periodic widths; the image rule is the forward's; z is not wrapped)
 *     reciprocal   k = 2 pi (m0 g_a + m1 g_b) != 0, |k| <= kc, k = |k|, u = k / (2 beta):
 *                  F+(k, z) = e^{ k z} erfc(u + beta z),   F-(k, z) = e^{-k z} erfc(u - beta z)
 *                  phi_i  += sum_k (pi / (A k)) sum_j q_j cos(k . d_ij) [F+ + F-](k, z_ij)       (j over ALL atoms of the cell, j == i too)
 *                  ffix_i -= q_i sum_k (pi / (A k)) sum_j q_j { -k sin(k . d_ij) [F+ + F-] + nhat k cos(k . d_ij) [F+ - F-] }
 *                  (d[F+ + F-]/dz = k [F+ - F-]: the Gaussian terms cancel exactly; the half plane m1 > 0, or m1 == 0 and m0 > 0, is
 *                  summed with the weight doubled: the summand is even in k)
 *     k = 0        phi_i  += -(2 sqrt(pi) / A) sum_j q_j [ exp(-beta^2 z_ij^2) / beta + sqrt(pi) z_ij erf(beta z_ij) ]    (j == i too)
 *                  ffix_i -= q_i sum_j q_j nhat [ -(2 pi / A) erf(beta z_ij) ]
 *     self         phi_i  -= (2 beta / sqrt(pi)) q_i                        (there for alpha == 0 and alpha > 0 alike)
 *     energy       E = 1/2 sum_i q_i phi_i per cell;   f = ffix + fq,  fq_i = -sum_k phi_k dq_k/dr_i
 * all times ke.  F+- are evaluated without overflow or cancellation: with ex = exp(-u^2 - beta^2 z^2), ex erfcx(u +- beta z) for an
 * argument u +- beta z >= 0 and 2 exp(+-k z) - ex erfcx(|u +- beta z|) otherwise.
 * A charged slab: the model conserves Q, which need not be 0, and the formulas are applied as written whatever Q.  No neutralising
 * background exists in two dimensions (a uniform sheet's potential grows with |z|, it cannot be hidden in a constant): the k = 0 term
 * is the finite part of a charged sheet's potential, and the infinite constant proportional to Q that is dropped does not depend on
 * beta.  phi of a charged slab is therefore defined up to that constant, E up to Q times it; ffix, fq and f are not touched by it
 * (sum_i dq_i/dr = 0).
 * epnn_ewald_slab_params (host only, no handle, no device) holds the rule for one cell [3][3], that of epnn_ewald_params over the
 * two periodic rows: s = sqrt(-ln tol), rc = w_min / 2, beta = s / rc, capped at alpha where alpha > 0 (then rc = 0: no real-space
 * part), kc = 2 beta s, M_k = ceil(kc |a_k| / 2 pi) for the periodic rows and 0 for the open row.  out [6] = beta, rc, kc, M0, M1,
 * M2.  tol means what it means there (the same three bounds; measured 0.005 to 0.013 of them on a 12-atom sheared slab, neutral or
 * charged).  About 131 half-plane vectors at tol = 1e-6 in a near-square cell, whatever its size.  It refuses, by name: a cell with
 * three periodic rows (use epnn_coulomb_xyz_cell), with one or none (not built), dependent rows, an entry that is not finite,
 * alpha negative or not finite, tol outside (0, 1), and a k box (2 M0' + 1)(M1' + 1) above 2^16 slots, M0' and M1' the M of the two
 * periodic rows (every k slot meets every pair: extreme aspect ratios are refused, not served slowly).
 * epnn_coulomb_xyz_slab takes ewald [B][6] (host, float64, a row per cell as epnn_ewald_slab_params writes it), checks that
 * beta > 0, 0 <= rc <= w_min / 2 (rc == 0 only with beta == alpha > 0), that the open row's M is 0, that the two others are
 * integers of at least ceil(kc |a_k| / 2 pi), and the slot cap, and runs at exactly those values.
 * Exclusions: the list (npairs, ex_i, ex_j, ex_scale) has the meaning, the checks and the refusals of epnn_coulomb_xyz_cell_excl:
 * the one nearest image of a listed pair gets (s - 1) times its bare kappa_alpha term, whatever beta; a listed pair farther apart
 * than half the smaller periodic width is refused by name after the device pass.  npairs == 0 is allowed (the three pointers may
 * then be NULL): the slab call needs one entry, not two.  A list whose factors are all 1 gives the bits of the call without a list;
 * the outputs depend neither on the order of the list nor on which atom of a pair is named first.
 * Outputs (host): q_out[A], phi_out[A], e_out[B] float64 (per cell), f_out[A][3]; ffix_out and fq_out may each be NULL and the
 * other outputs have the same bits either way.  The strain derivative: epnn_coulomb_xyz_slab_strain below (one periodic axis is not built).
 * Contract: that of epnn_coulomb_xyz_cell, word for word where it applies: the pair-list path whatever "grad_path" says, no
 * training state touched, waits for a "train_async" step, the same refusals by name (coincident atoms or images included, a
 * periodic width below twice the cutoff, a molecule that does not fit N), the handle left usable; h_dim below 48 zero-padded; no
 * float atomics and every sum in a fixed order; a cell's rows depend neither on the rest of the batch nor on the order of the list.
 * Bits: q_out has the bits of epnn_charges_vjp_xyz_cell on "grad_path" 2 with the same cell; fq_out is bit for bit -gxyz_out of
 * that entry called with g = phi_out; f_out == ffix_out + fq_out in float32.
 * Arithmetic: the real-space part is epnn_coulomb_xyz_cell's sweep as it is.  The reciprocal and k = 0 part is one all-pairs sweep
 * on the open sweep's tasks in which every pair meets every slot of its cell's half plane (listed by the host in float64, with
 * exp(-u^2) folded into the weight).  Per pair z_ij, the two fractional differences and exp(-beta^2 z^2) are float64; per (pair,
 * slot) the phase 2 pi frac(m0 f0 + m1 f1) and the two erfc arguments are taken in float64 and rounded once, and the exponent of
 * 2 exp(+-k z) is split into two float32; everything else is float32 (sincosf, erfcxf, expf, erff, the products); the running sums
 * are float64.  phi, ffix and E are each within 2e-6 of the sum of their absolute real-space terms (and of the listed pairs'
 * correction terms), plus 41 * 2^-24 of their absolute reciprocal terms (pi / (A k)) [F+ + F-] |q_j|, for ffix k times that, plus
 * 16 * 2^-24 of their absolute k = 0 terms (tests/test_gpu_coulomb_slab.py counts the roundings; measured: 0.036 of that at worst).
 * Device scratch (epnn_last_stats out[2]): that of epnn_coulomb_xyz on the same batch (both formulas there) plus what the slab adds
 * -- the real-space rows are [cpieces][A][10] instead of [cpieces][A][4], the reciprocal sweep's rows [cpieces][A][5], and staged
 * with the inputs the cells' records (120 B), the two sweeps' parameters (72 B and 112 B) and the slots:
 *     bytes = epnn_coulomb_xyz's + 88 A cpieces + 304 B + 56 slots                (the 72 B rounded up to a multiple of 16)
 * cpieces and ctasks as at epnn_coulomb_xyz, slots = the batch's listed half-plane slots; with a list of P pairs, P > 0, also
 * (A + 1) 4 + 16 P + 80 A (two buffers).  Time grows as n^2 times the slots: the exact method's price. */
int epnn_ewald_slab_params(const float *cell, double alpha, double tol, double *out);
int epnn_coulomb_xyz_slab(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                          const float *cell, const double *ewald, double ke, double alpha, int64_t npairs, const int32_t *ex_i,
                          const int32_t *ex_j, const float *ex_scale, float *q_out, float *phi_out, double *e_out, float *f_out,
                          float *ffix_out, float *fq_out);
/* ---- the strain derivative of the slab sum: epnn_coulomb_xyz_slab with the strain outputs of epnn_coulomb_xyz_cell_excl (in-plane
 * pressure coupling, fixed surface tension; INTEGRATION.md, "Slabs").  gstrain [B][3][3] = dE/d eps under r -> (1 + eps) r and
 * a_k -> (1 + eps) a_k for the two periodic rows, eps symmetric: the strain of epnn_charges_vjp_xyz_cell.  beta, rc, kc, the listed
 * slots (m0, m1) and the set of in-range pairs are held fixed, as in the periodic call.  To first order A -> A (1 + tr eps - n eps n),
 * k -> k - (k eps k) / k, z_ij -> z_ij (1 + n eps n), and the phase k . d_ij changes by 2 z_ij (n eps k): a symmetric out-of-plane
 * shear tilts the plane and the in-plane dual vectors stay in it.  In the notation above, c = pi / (A k) over the whole plane,
 * Fs = F+ + F-, Fd = F+ - F-, theta = k . d_ij:   dFs/dz = k Fd;   dFs/dk = z Fd - (2 / (beta sqrt(pi))) exp(-u^2 - beta^2 z^2);
 *     gstrain_fix_ab = -(E_rec + E_k0) (delta_ab - n_a n_b)
 *                      + 1/2 sum_ij q_i q_j sum_k c cos(theta) [Fs / k^2 - (dFs/dk) / k] k_a k_b
 *                      + n_a n_b 1/2 sum_ij q_i q_j z_ij { sum_k c k cos(theta) Fd - (2 pi / A) erf(beta z_ij) }
 *                      - 1/2 sum_ij q_i q_j z_ij sum_k c sin(theta) Fs (n_a k_b + k_a n_b)                       (j == i included)
 *                      + 1/2 sum_{i != j} q_i q_j kappa_s'(D) d_a d_b / D  +  sum_listed (s - 1) q_i q_j kappa_alpha'(D) d_a d_b / D
 * all times ke; E_rec and E_k0 the reciprocal and k = 0 parts of E.  The self term has no strain and there is no background term.
 * gstrain_q_ab = sum_k phi_k dq_k/d eps_ab, the backward's strain rows, and gstrain = gstrain_fix + gstrain_q.
 * Arguments: those of epnn_coulomb_xyz_slab, with the outputs of epnn_coulomb_xyz_cell_excl.  gstrain_out [B][3][3] is required;
 * ffix_out, fq_out, gstrain_fix_out and gstrain_q_out may each be NULL.  Contract, checks and refusals: epnn_coulomb_xyz_slab's, word
 * for word.  epnn_coulomb_xyz_slab itself keeps its kernels, bits and scratch.
 * Bits: q, phi, e, f, ffix and fq are those of epnn_coulomb_xyz_slab on the same inputs; gstrain_q_out is bit for bit gstrain_out of
 * epnn_charges_vjp_xyz_cell on "grad_path" 2 called with g = phi_out; gstrain == gstrain_fix + gstrain_q in float32, and each is
 * bitwise symmetric (six sums mirrored into nine slots).
 * Arithmetic: the reciprocal and k = 0 sums have no structure factor, so their strain rides in the all-pairs sweep: six more float64
 * sums per lane beside the five, in the basis of the slot integers (the z-weighted force along nhat; the z-weighted in-plane force
 * times m0, m1; the bracket above times m0^2, m0 m1, m1^2), float32 products of values the sweep already has and no new
 * transcendental; the atoms' kernel expands them through g_a, g_b and nhat in float64 and adds the virial rows of the real-space sweep
 * and of the listed pairs; one wavefront per cell adds the atoms' shares.  No float atomics, every sum in a fixed order.
 * Accuracy: every component of gstrain_fix is within 2e-6 of its absolute real-space and listed pairs' terms, plus 43 * 2^-24 of its
 * absolute reciprocal terms, plus 16 * 2^-24 of its absolute k = 0 terms, plus 2 * 2^-24 of its own size (tests/
 * test_gpu_coulomb_slab_strain.py counts the roundings and tests/slab_strain_ref.py defines the absolute terms: those of the formula
 * above with |Fd| counted as Fs and k_a, k_a k_b counted in the slot integers' basis).
 * Device scratch (epnn_last_stats out[2]): epnn_coulomb_xyz_slab's on the same batch and list, plus the wider rows of the sweep
 * ([cpieces][A][11] instead of [5]), the atoms' strain shares [A][6] and the [B][9] fixed-charge rows behind E:
 *     bytes = epnn_coulomb_xyz_slab's + 48 A cpieces + 48 A + 36 B */
int epnn_coulomb_xyz_slab_strain(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                                 const float *cell, const double *ewald, double ke, double alpha, int64_t npairs, const int32_t *ex_i,
                                 const int32_t *ex_j, const float *ex_scale, float *q_out, float *phi_out, double *e_out, float *f_out,
                                 float *gstrain_out, float *ffix_out, float *fq_out, float *gstrain_fix_out, float *gstrain_q_out);
/* ---- per-atom Gaussian widths, self-energy and on-site terms in slab cells: the energy of epnn_coulomb_xyz_site / _cell_site (its
 * block above has E, gamma_ij, the new inputs sigma, chi, hard, self_term and what they mean) for two periodic axes and one open one.
 * epnn_coulomb_xyz_slab_site takes epnn_coulomb_xyz_slab's arguments with sigma, chi, hard, self_term behind alpha and mu_out behind
 * phi_out, epnn_coulomb_xyz_slab_strain_site the same on epnn_coulomb_xyz_slab_strain: the order of epnn_coulomb_xyz_cell_site.  The
 * sum of epnn_coulomb_xyz_slab (its notation) changes as follows:
 *     real         kappa_s(D) = [erf(gamma_ij D) - erf(beta D)] / D over the minimum image, D <= rc; with sigma NULL gamma_ij is alpha
 *     reciprocal, k = 0 and the split's self term -(2 beta / sqrt(pi)) q_i: the point charges' sums, unchanged
 *     self         [self_term]  phi_i += 2 gamma_ii q_i / sqrt(pi),   gamma_ii = 1 / (2 sigma_i), or alpha when sigma is NULL
 *     listed       (s - 1) times the bare erf(gamma_ij D) / D term of the one nearest image, whatever beta
 *     mu_i   = chi_i + J_i q_i + phi_i                        = dE/dq_i, the seed of the backward
 *     E      = sum_i [ chi_i q_i + 1/2 J_i q_i^2 + 1/2 q_i phi_i ]   per cell (float64)
 *     fq_i   = -sum_k mu_k dq_k/dr_i,     f = ffix + fq
 * all of phi times ke; chi and J are not multiplied by ke.  There is no background term and no per-pair k = 0 correction, for charged
 * slabs too, and this is the one point where the slab differs from epnn_coulomb_xyz_cell_site: the Gaussians' sum equals the point
 * charges' sum minus sum over images erfc(gamma_ij D) / D, that difference is short-ranged and is summed in real space (the real term
 * above, inside the width check), and the constant dropped for a charged sheet depends on neither beta nor gamma.  (tests/
 * test_slab_site_ref.py pins it: E equals the Gaussians' own two-dimensional sum, the reciprocal and k = 0 formulas with beta = gamma_ij
 * per pair, for Q = 0 and Q != 0.)
 * Strain: gstrain_fix of epnn_coulomb_xyz_slab_strain with the new kappa_s' in the real-space virial and kappa_gamma' in the listed
 * pairs' virial; the self and on-site terms have no strain and nothing is added for a background.  gstrain_q = sum_k mu_k dq_k/d eps
 * comes from the backward's strain rows, and gstrain = gstrain_fix + gstrain_q.
 * Width check: a cell whose gamma_min = 1 / (2 sigma_max) is below its row's beta is refused by name, in the words of
 * epnn_coulomb_xyz_cell_site: the cell, sigma_max and the largest width 1 / (2 beta) allowed.  With widths the caller takes
 * epnn_ewald_slab_params(cell, 0, tol); sigma NULL with alpha > 0 keeps the existing rule (beta capped at alpha, rc = 0).
 * Refusals: those of the _site entries above, word for word (sigma with alpha > 0; a sigma that is zero, negative or not finite, or
 * whose 2 sigma^2 is not a positive finite float32; chi or hard not finite; self_term other than 0 or 1, or 1 with neither sigma nor
 * alpha > 0; the width check), and everything epnn_coulomb_xyz_slab refuses (cubes, wires, the row checks, the list's checks, a listed
 * pair beyond half the smaller width); the handle stays usable.  Contract otherwise: epnn_coulomb_xyz_slab's, word for word.
 * Outputs: those of the slab entries plus mu_out[A]; mu_out, ffix_out, fq_out, gstrain_fix_out and gstrain_q_out may each be NULL and
 * the other outputs have the same bits either way (gstrain_out is required by the strain entry).
 * Bits: q_out has the bits of epnn_charges_vjp_xyz_cell on "grad_path" 2; fq_out and gstrain_q_out are bit for bit -gxyz_out and
 * gstrain_out of that entry called with g = mu_out; f == ffix + fq and gstrain == gstrain_fix + gstrain_q in float32; gstrain_fix and
 * gstrain are bitwise symmetric; q, phi, mu, e, f, ffix and fq of the strain entry are those of the plain one.  With sigma, chi and
 * hard all NULL and self_term = 0 the call runs the existing slab kernels: every output has the bits of epnn_coulomb_xyz_slab /
 * _slab_strain on the same arguments, and mu_out == phi_out.
 * Arithmetic: the real-space sweep with widths is epnn_coulomb_xyz_cell_site's (k_ew_sweep_site, with its virial sums), the listed
 * pairs' kernel its widths mode through the minimum image; the reciprocal and k = 0 sweeps are the slab entries' as they are.  The
 * atoms' kernels get a site form: they add the Gaussian self term to phi behind the split's, write mu into the seed and into mu_out,
 * and q (chi + 1/2 J q) + 1/2 q phi into the energy share, in float64, as the open and periodic site kernels do.  The bounds of the
 * slab entries hold with 2 * 2^-24 more of the self and on-site terms (the rounding of phi and mu to float32).
 * Device scratch (epnn_last_stats out[2]) when any of sigma, chi, hard, self_term is given: the slab entry's on the same batch and
 * list (epnn_coulomb_xyz_slab's, or _slab_strain's) plus the staged rows [A] float4, one buffer more (plus up to 256 of rounding), and
 * mu [A] at the end of the outputs' buffer; slabs have no per-cell sum:
 *     bytes = the slab entry's + 16 A + 4 A */
int epnn_coulomb_xyz_slab_site(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                               const float *cell, const double *ewald, double ke, double alpha, const float *sigma, const float *chi,
                               const float *hard, int self_term, int64_t npairs, const int32_t *ex_i, const int32_t *ex_j,
                               const float *ex_scale, float *q_out, float *phi_out, float *mu_out, double *e_out, float *f_out,
                               float *ffix_out, float *fq_out);
int epnn_coulomb_xyz_slab_strain_site(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                                      const float *cell, const double *ewald, double ke, double alpha, const float *sigma, const float *chi,
                                      const float *hard, int self_term, int64_t npairs, const int32_t *ex_i, const int32_t *ex_j,
                                      const float *ex_scale, float *q_out, float *phi_out, float *mu_out, double *e_out, float *f_out,
                                      float *gstrain_out, float *ffix_out, float *fq_out, float *gstrain_fix_out, float *gstrain_q_out);
/* ---- training on periodic and large systems. epnn_train_step_xyz with a cell: cell [B][3][3] (host) has exactly the meaning and
 * the checks of epnn_forward_xyz_cell (zero rows are open axes, a perpendicular width below 2 * cutoff is refused, a diagonal cell
 * is an orthorhombic box), NULL means open molecules.  Loss = sum (y - p)^2 over the real atoms; the gradient goes into the handle's
 * flat vector (epnn_get_gradients); apply != 0 adds the guarded all-reduce and the Adam step, as in epnn_train_step_xyz.  Two
 * implementations stand behind it (option "train_path"): the dense path -- epnn_train_step_xyz's kernels on rows padded to
 * [B][N][N] whose distances are minimum-image ones, with "train_fused", "train_async" and "train_graph" as there -- and the
 * pair-list path: the checkpointed forward and the backward of epnn_charges_vjp_xyz's pair-list path seeded with 2 (q - y), with
 * the weight gradients summed per atom, per listed pair and, for the second Dense of a message MLP, over all pairs inside the
 * backward sweep (f32 MFMA).  The pair-list path reads the device masters directly, keeps per-atom rows and the listed pairs only
 * (scratch O(atoms + listed pairs) plus constant-size partial sums; profiles/r10_train_large.txt), is bit-reproducible (no atomics,
 * every sum in a fixed order), waits for a dense "train_async" step still in flight, and returns when all of it is done: it has
 * to wait for the pair count once anyway, so "train_async" and "train_graph" do not apply to it.  It is built for update layers
 * [32, 32] on a handle without epnn_set_partition.  After a call on it epnn_last_stats gives out[0] = listed pairs, out[1] = 0,
 * out[2] = bytes of device scratch the call used.  epnn_train_step_xyz itself never takes the pair-list path. */
int epnn_train_step_xyz_cell(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                             const float *cell, const float *y_flat, float *q_out_flat, float *loss_out, int apply);
/* RCCL communicator (one rank per GPU): the gradient is summed with ONE ncclAllReduce of the flat vector; the same
 * communicator carries the row exchange of a partitioned large system (epnn_set_partition with exchange == NULL). */
int epnn_comm_unique_id(char *out128);
int epnn_comm_init(epnn_handle *h, const char *id128, int rank, int world);
/* ranks that joined the communicator (ncclCommCount) */
int epnn_comm_count(epnn_handle *h, int32_t *ranks_out);
/* all-reduce of n <= 1024 host doubles over the communicator, on the handle's stream, waited for (op 0 = sum, 1 = max): the
 * barrier and the MAX-over-ranks timing of a multi-process driver go through the same RCCL path as the product's collectives
 * (the reference has nothing distributed; bench.py --gpus N is the caller) */
int epnn_comm_allreduce(epnn_handle *h, double *inout, int32_t n, int32_t op);

/* (tests) the pair list of the last forward that built one outside the fused kernel: first / second atom and near weight
 * (is_near of charge_gn.py:90-94 as 1.0 / 0.0, times the mask for dense inputs) of up to `cap` pairs; *count_out = pairs listed */
int epnn_debug_pairs(epnn_handle *h, int32_t *pi, int32_t *pj, float *pwi, int64_t cap, int64_t *count_out);

/* Device memory and stream plumbing for callers that keep inputs resident (bench.py). */
int epnn_dev_alloc(epnn_handle *h, size_t bytes, void **out);
int epnn_dev_free(epnn_handle *h, void *p);
int epnn_memcpy_h2d(epnn_handle *h, void *dst, const void *src, size_t bytes);
int epnn_memcpy_d2h(epnn_handle *h, void *dst, const void *src, size_t bytes);
int epnn_sync(epnn_handle *h);

/* hipEvent timing on the handle's stream: begin/end bracket any number of calls; elapsed in ms.
 * epnn_last_timing: per-stage device times of the most recent forward when profiling is enabled with
 * epnn_set_option("profile", k): out[0]=front-end, out[1]=fused small-molecule kernel, out[2]=tiled
 * large-system kernels, out[3]=total. (infer.py:70-79 prints wall-clock; this is the device-side view.) */
int epnn_timer_begin(epnn_handle *h);
int epnn_timer_end(epnn_handle *h, float *elapsed_ms);
int epnn_last_timing(epnn_handle *h, float *out4);
/* same for the idx-th forward issued since "profile" was set (pool of that many event sets; no sync in between). */
int epnn_timing_at(epnn_handle *h, int idx, float *out4);
/* Options a caller may want to touch (every other name epnn_set_option accepts is a developer switch that selects between
 * implementations with identical results: include/epnn_dev.h).  Unknown names and out-of-range values fail.
 *   "profile"           0 = off (default); k > 0: keep the stage events of the last k forwards (epnn_timing_at)
 *   "force_path"        0 = by molecule size (default); 1 = fused small-molecule kernels only (fails above 32 atoms); 2 = tiled kernels only
 *   "pair_cap_per_atom" initial capacity of the near-pair list of the tiled / dense paths (it grows by itself; default 16)
 *   "wave2"             how batches of small molecules use the block-per-wavefront kernel: -1 (default) = molecules of 17..32 atoms
 *                       on two wavefronts and smaller ones two to a workgroup when the batch has at most 1024 molecules (halves the
 *                       latency of a lone batch); 0 = one wavefront per molecule throughout (set on handles whose launches overlap:
 *                       engine.Pipeline does); 17..32 = split from that many atoms
 *   "wave3"             1 (default) = molecules of 33..48 / 49..64 atoms run on three / four wavefronts of the fused kernel; 0 = on the
 *                       tiled kernels
 *   "sync_spin_us"      epnn_sync and every call that waits for a forward poll the stream this many microseconds (yielding the core
 *                       between polls) before they sleep on its completion; default 2000, 0 = sleep at once
 *   "large_dedupe"      1 (default) = the tiled path's first GNN step of the compact entry groups the atoms by feature row (h = 0 and one
 *                       q per molecule there: the all-pairs sum of charge_gn.py:70 takes (distinct rows)^2 pair evaluations instead of
 *                       n^2; a molecule with more than 64 distinct rows switches the handle back by itself); 0 = always the all-pairs sweep
 *   "train_fused"       1 (default) = train step with one workgroup per atom and pair MLP, Dense layers and weight gradients as f32
 *                       MFMA tiles, 2T + 2T + 1 launches; 0 = one launch per Dense layer on materialised rows (also taken above 96
 *                       atoms and for update layers other than [32, 32])
 *   "grad_path"         which implementation epnn_charges_vjp_xyz and its _pbc / _cell forms run: 0 (default) = the dense path while
 *                       B N^2 <= 2^22 (every call that fitted a GPU before takes the path it took, bit for bit), the pair-list path
 *                       above that; 1 = always the dense path; 2 = always the pair-list path (refused by name for update layers other
 *                       than [32, 32] and on a partitioned handle, which stay on the dense path under 0)
 *   "train_path"        which implementation epnn_train_step_xyz_cell runs (epnn_train_step_xyz always runs the dense one): 0 (default) =
 *                       the dense path while B N^2 <= 2^22, the pair-list path above that; 1 = always the dense path; 2 = always the
 *                       pair-list path (refused by name for update layers other than [32, 32] and on a partitioned handle, which
 *                       stay on the dense path under 0)
 *   "train_async"       1 (default) = a training step returns as soon as its forward pass is done (loss and predictions are on the host
 *                       then; backward and optimizer keep running, every call that reads weights or gradients waits for them); 0 = a
 *                       step returns when all of it is done
 *   "train_graph"       1 (default) = a train step that waits for its own end has its launch sequence captured once per (B, N, buffers)
 *                       and replayed as a hipGraph; 0 = kernel by kernel */
int epnn_set_option(epnn_handle *h, const char *name, int value);
/* The fused kernel's own front-end runs its G products in a 16-dimensional basis of the Gaussian edge features
 * (charge_gn.py:148-161: 48 overlapping bumps of one variable).  Returns max |e - B B^T e| over D in [0, cutoff], relative
 * to max e = 1 (5e-10 for cutoff 3, eta 2); the basis is used only when this is below 1e-8. */
double epnn_edge_basis_residual(epnn_handle *h);
/* counters of the most recent forward: out[0]=listed pairs (unordered, D < cutoff; the is_near test of charge_gn.py:90-94
 * enters as the pairs' weights), out[1]=molecules on the fused path,
 * out[2]=molecules on the tiled path, out[3]=pair-list regrows, plus forwards in which a wavefront of the fused kernel left the clamp form
 * of the first ReLU for a step (its scaled rows beyond the clamp's range: see "arithmetic" at the top; the results are the same bits). */
int epnn_last_stats(epnn_handle *h, int64_t *out4);

#ifdef __cplusplus
}
#endif
#endif /* EPNN_H */
