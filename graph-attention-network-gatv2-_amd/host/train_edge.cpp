// train_edge — drop-in for the reference's edge-based GATv2 trainer (GATv2_edge_based.cu `main`,
// cited E:<line>): same command-line flags and defaults, same four-text-file CSR dataset, same
// stdout/stderr lines, but every device operation goes through the C ABI of include/gatv2_abi.h
// (libgatv2_hip.so: hand-written HIP for MI355X).  This file is plain host C++: no HIP headers.
//
//   ./train_edge --dataset cora --data-root /path/to/datasets --num-layers 2 --heads 8,8 ...
//                --outdims 8,8 --epochs 20 --optimizer adam --lr 0.01 --clip
//
// Additive flags (not in the reference): --seed N (parameter init; default time(NULL) like
// E:1305), --load-params FILE / --dump-params FILE (raw fp32: W | a | Wo in the reference
// layouts), --device N, --cache (binary cache of the parsed text files, written next to them),
// --ranks P [--transport rccl|host]: destination-range sharding over P GPUs of the node, one forked
// process per GPU (devices --device .. --device+P-1), exchanges inside the library (RCCL over xGMI;
// "host" stages them through shared memory and lets ranks share a GPU — for testing).  Every rank
// reads the dataset, keeps its destination range (host/shard_plan.h) and the replicated input
// features; rank 0 prints.  Same numbers as one GPU up to fp32 summation order.
// --halo 0|1|2 (with --ranks): the table exchanges move only the rows the receiving shard's edges reference (gat_comm_option
// GAT_COMM_HALO; 2 = only where fewer than half of the rows would travel).  Same numbers as the full exchange.
// --dtype f32|bf16: storage type of the gathered / exchanged source table and the per-edge message
// rows (arithmetic stays fp32).
// --dropout P / --attn-dropout P (default 0): inverted dropout on every layer's input features / on the attention
// coefficients during training (gatv2_abi.h "dropout"), masks keyed by --seed.  With --val-mask the validation line
// then comes from an eval-mode forward (no dropout) after the optimizer step.  Both 0: the output is the reference's.
// --drop-edge P (default 0): DropEdge (gatv2_abi.h "DropEdge"): every training step drops each edge with probability P BEFORE the
// softmax, masks keyed by --seed; --drop-edge-keep-self never drops self-loops, --drop-edge-shared draws one mask per step for all
// layers.  Validation (--val-mask) then comes from an eval-mode forward, as with dropout.
// --residual / --bias: every layer adds Wres x' / b to h_pre (gatv2_abi.h "residual"); Wres is Xavier-initialised from --seed after the
// other parameters (which keep their values), b starts at 0.  --dump-params / --load-params then carry the groups Wres and b behind
// W, a and Wo — only the groups whose flag is on, so files written without the flags keep their format.
// --layer-norm [--norm-eps X] [--norm-skip-last]: LayerNorm over each row's H*D channels between the aggregation and the LeakyReLU
// (gatv2_abi.h "layer normalisation"; eps default 1e-5; --norm-skip-last leaves the last layer un-normalised); gamma starts at 1, beta
// at 0, and --dump-params / --load-params carry gamma and beta behind the residual groups, only with the flag.
// --batch-norm [--bn-momentum M] [--norm-eps X] [--norm-skip-last]: BatchNorm over the columns of each layer's [N][H*D] aggregate between the
// aggregation and the LeakyReLU (gatv2_abi.h "batch normalisation"; momentum default 0.1; not together with --layer-norm; one rank).
// Validation (--val-mask) then comes from an eval-mode forward, on the running statistics.  gamma and beta travel in --dump-params /
// --load-params as with --layer-norm, and — only with this flag — running_mean then running_var follow the last group.
// --edge-features: per-edge attributes in the attention score (gatv2_abi.h "edge features"): edge_features.txt of the dataset folder holds
// E lines of Fe values, line j for CSR edge j (Fe is derived from the count); We is Xavier-initialised from --seed after every other
// parameter, and --dump-params / --load-params carry We behind beta, only with the flag.  CSR datasets as they are, one rank: the flag
// is refused with an edges.txt dataset, with --add-self-loops / --undirected / --coalesce (the graph would be rebuilt and the rows
// would no longer match its edges) and with --ranks > 1.
// --readout mean|sum|max: graph classification (gatv2_abi.h "graph-level readout"): the dataset is a batch of graphs packed block-diagonally
// into one CSR, graph_ptr.txt of the dataset folder holds G+1 integers (graph g owns nodes graph_ptr[g] .. graph_ptr[g+1]-1), and
// labels.txt, --train-mask and --val-mask files hold G lines.  The last layer's rows are pooled per graph in front of the output head;
// the epoch lines keep their format, loss and accuracy are over graphs.  One rank only (a graph may straddle shards); --cache is not used.
// --pairs mul|add: link prediction / edge classification (gatv2_abi.h "pair head"): pairs.txt of the dataset folder holds one node pair
// "u v" per line (not necessarily an edge), labels.txt / targets.txt, --train-mask and --val-mask files hold one line per pair.  The output
// head reads X[u]*X[v] / X[u]+X[v] of the last layer's rows; the epoch lines keep their format, loss and accuracy are over pairs.  One rank
// only (an endpoint may live on another shard), not with --readout; --cache is not used.
// --head-hidden K [--head-act relu|lrelu]: one hidden layer of K units in front of the output head (gatv2_abi.h "hidden layer"), for every
// head kind: Z1 = act(Xin W1^T + b1), the head reads Z1 and Wo becomes [C][K]; act is ReLU, or LeakyReLU with the model's slope.  W1 is
// Xavier-initialised from --seed after every other parameter, b1 starts at 0, and --dump-params / --load-params carry W1 and b1 behind We,
// only with the flag (files written without it keep their format).  One rank only: refused with --ranks > 1 before any GPU call.
// --rank-metrics K1,K2,... (with --val-mask, --ranks 1, not --loss mse): one more line behind every validation line — ROC-AUC, average
// precision, MRR and Hits@K of the validation rows (gatv2_abi.h "ranking metrics"), macro-averaged over the output columns that have both
// classes, then the count of those columns.  Every other line is printed as without the flag.
// --weight-decay X, --optimizer adamw, --momentum M [--nesterov], --clip-global T, --no-decay-bias-norm, --fused-step: the update runs on
// the device-side optimizer (gatv2_abi.h "optimizer step on the device": gat_set_optimizer once, then gat_optimizer_step in place of
// gat_clip + gat_step_*; --clip becomes its per-group clip at 5, --clip-global its global-norm clip; --no-decay-bias-norm clears the decay
// bits of b, gamma, beta and b1).  --fused-step makes the epoch body the one call gat_train_step (on one rank a replayed graph) and moves
// the validation line behind the update, from a forward of its own.  Bad values are refused with the usage text before any GPU call.
// With none of these flags the program makes the reference's calls and prints the reference's text.
// --add-self-loops / --undirected / --coalesce: the graph is rebuilt on the device before training (gat_graph_from_coo:
// GAT_GRAPH_SELF_LOOPS / SYMMETRIZE / COALESCE, applied in that order); a CSR dataset is expanded to an edge list first.
// Edge-list dataset: a folder with edges.txt (one "src dst" pair per line, a message flows src -> dst) instead of
// row_ptr.txt / col_idx.txt is read and built the same way.  The flags and the resulting edge count are printed once.
// With --ranks P > 1 the build runs in one short-lived forked child (the parent never touches the HIP runtime) that hands
// the CSR back through shared memory.  --cache applies to CSR datasets (the files as read; the flags apply after loading).
// --help prints the usage text.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include <signal.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>

#include "gatv2_abi.h"
#include "shard_plan.h"

namespace {

struct Options {
    int epochs = 200;                 // E:935
    int layers = 2;                   // E:936
    bool clip = false;                // E:937
    std::string optimizer = "sgd";    // E:938
    float lr = 0.0001f, beta1 = 0.9f, beta2 = 0.999f;   // E:939
    bool beta1_given = false, beta2_given = false;
    std::vector<int32_t> heads, outdims;
    bool heads_given = false, outdims_given = false;
    std::string dataset = "pubmed";   // E:1050
    std::string data_root = "./data"; // E:1051
    // additive
    uint64_t seed = 0; bool seed_given = false;
    std::string load_params, dump_params;
    int device = 0;
    bool cache = false;
    int ranks = 1;
    std::string transport = "rccl";
    int halo = 0;
    std::string dtype = "f32";
    std::string train_mask, val_mask;     // text files of N 0/1 values (beyond the reference: README R:134 "later")
    float dropout = 0.f, attn_dropout = 0.f;
    float drop_edge = 0.f; int drop_edge_flags = 0;   // GAT_DROPEDGE_*: --drop-edge-keep-self, --drop-edge-shared
    int residual_flags = 0;                           // GAT_RES_*: --residual, --bias
    int norm_flags = 0; float norm_eps = 1e-5f;       // GAT_NORM_*: --layer-norm, --norm-skip-last; --norm-eps
    bool batch_norm = false; float bn_momentum = 0.1f; // --batch-norm, --bn-momentum (eps and skip-last: the two norm flags above)
    int graph_flags = 0;                  // GAT_GRAPH_*: --add-self-loops, --undirected, --coalesce
    std::string readout;                  // --readout mean|sum|max: graph_ptr.txt of the dataset folder, one label per graph
    bool edge_features = false;           // --edge-features: edge_features.txt of the dataset folder enters the attention score
    std::string pairs;                    // --pairs mul|add: pairs.txt of the dataset folder ("u v" per line), one label per pair
    std::string neg_sampling;             // --neg-sampling uniform|corrupt: lines --neg-first .. of pairs.txt are redrawn before every epoch
    long long neg_first = -1; uint64_t neg_seed = 0; int neg_flags = 0;      // --neg-first K, --neg-seed S, GAT_NEG_*: --neg-both-directions, --neg-allow-self
    std::string loss = "softmax";         // --loss softmax|bce|mse: bce / mse read targets.txt (rows of C floats, nan allowed) in place of labels.txt
    int head_hidden = 0; int head_act = 0;   // --head-hidden K, --head-act relu|lrelu (GAT_HEAD_ACT_*): a hidden layer in front of the output head
    std::vector<int32_t> rank_ks; bool rank_metrics = false;      // --rank-metrics K1,K2,...: a ranking line behind every validation line
    // the optimizer on the device (gatv2_abi.h "optimizer"): any of these flags moves the update from gat_clip / gat_step_* to gat_set_optimizer
    float weight_decay = 0.f, momentum = 0.f, clip_global = 0.f;  // --weight-decay X, --momentum M, --clip-global T
    bool nesterov = false, no_decay_bias_norm = false, fused_step = false;   // --nesterov, --no-decay-bias-norm, --fused-step
    bool device_optimizer() const { return weight_decay > 0.f || momentum > 0.f || clip_global > 0.f || nesterov || no_decay_bias_norm || fused_step || optimizer == "adamw"; }
};

// A CSR built before the ranks were forked (main): row_ptr [n + 1] then col_idx [e] in shared memory.
struct Prebuilt { const int32_t* row_ptr = nullptr; const int32_t* col_idx = nullptr; int64_t n = 0, e = 0, n_in = 0; };

const char* kUsage =
    "Usage: train_edge --heads H1,..,HL --outdims D1,..,DL [--num-layers L] [--epochs N] [--optimizer sgd|adam] [--lr X]\n"
    "                  [--beta1 X] [--beta2 X] [--clip] [--dataset NAME] [--data-root DIR]\n"
    "  dataset folder: features.txt, labels.txt and either row_ptr.txt + col_idx.txt (CSR, rows = destinations)\n"
    "                  or edges.txt (one \"src dst\" pair per line)\n"
    "  graph:    --add-self-loops   every node ends with exactly one self-loop (existing ones are replaced)\n"
    "            --undirected       add the reverse of every edge\n"
    "            --coalesce         reduce duplicate edges to one\n"
    "            (applied in this order, on the device, before training; with --ranks to the whole graph)\n"
    "  additive: --seed N --load-params FILE --dump-params FILE --device N --cache --dtype f32|bf16\n"
    "            --train-mask FILE --val-mask FILE --dropout P --attn-dropout P\n"
    "            --drop-edge P [--drop-edge-keep-self] [--drop-edge-shared]   DropEdge: each training step drops every edge with\n"
    "                          probability P before the softmax (never a self-loop / one mask for all layers instead of one per layer)\n"
    "            --residual         every layer adds Wres x' to h_pre (a skip connection through a learned linear map)\n"
    "            --bias             every layer adds a learned bias b to h_pre\n"
    "                          (--dump-params / --load-params then append Wres and b behind W, a and Wo)\n"
    "            --layer-norm [--norm-eps X] [--norm-skip-last]   LayerNorm over each row's H*D channels before the LeakyReLU\n"
    "            --batch-norm [--bn-momentum M] [--norm-eps X] [--norm-skip-last]   BatchNorm over each layer's columns (all nodes) before the LeakyReLU\n"
    "                          (eps X, default 1e-5 / not in the last layer; gamma and beta follow b in --dump-params / --load-params)\n"
    "            --edge-features    per-edge attributes enter the attention score: edge_features.txt of the dataset folder, E lines of Fe\n"
    "                          values in CSR order (CSR datasets only, not with the graph flags, --ranks 1; We follows beta in\n"
    "                          --dump-params / --load-params)\n"
    "            --readout mean|sum|max   graph classification: graph_ptr.txt of the dataset folder holds G+1 integers (graph g owns nodes\n"
    "                          graph_ptr[g] .. graph_ptr[g+1]-1); labels.txt, --train-mask and --val-mask then hold G lines; the last\n"
    "                          layer's rows are pooled per graph before the output head; loss and accuracy are over graphs (--ranks 1)\n"
    "            --pairs mul|add    link prediction / edge classification: pairs.txt of the dataset folder holds one node pair \"u v\" per\n"
    "                          line (pairs need not be edges); the output head reads X[u]*X[v] (mul) or X[u]+X[v] (add) of the last\n"
    "                          layer's rows; labels.txt / targets.txt, --train-mask and --val-mask then hold one line per pair; loss and\n"
    "                          accuracy are over pairs (--ranks 1, not with --readout)\n"
    "            --neg-sampling uniform|corrupt --neg-first K [--neg-seed S] [--neg-both-directions] [--neg-allow-self]   with --pairs:\n"
    "                          lines K.. of pairs.txt are negative slots, redrawn on the device before every epoch (round = epoch index)\n"
    "                          as node pairs that are not edges of the graph — uniform, or one endpoint of a pair of lines 0..K-1\n"
    "                          replaced (corrupt); not an edge in either direction / self pairs allowed with the two flags\n"
    "            --loss softmax|bce|mse   the output head's loss (default softmax: labels.txt as always).  bce (multi-label) and mse\n"
    "                          (regression) read targets.txt in place of labels.txt: one row of C floats per node — per graph with\n"
    "                          --readout — where nan marks a missing entry; C is the row width.  The epoch line prints the loss sum over\n"
    "                          the present entries of the training rows, and for bce the accuracy over those entries\n"
    "            --head-hidden K [--head-act relu|lrelu]   one hidden layer of K units in front of the output head (an MLP predictor, for\n"
    "                          node, --readout and --pairs heads alike): Z1 = act(Xin W1^T + b1), act = ReLU (default) or LeakyReLU with the\n"
    "                          model's slope; W1 and b1 follow We in --dump-params / --load-params, only with the flag (--ranks 1)\n"
    "            --rank-metrics K1,K2,...   with --val-mask: behind every validation line one line \"Val AUC: .., AP: .., MRR: .., Hits@K1: ..\n"
    "                          (n columns)\" — ROC-AUC, average precision, MRR (every positive against all negatives) and Hits@K of the\n"
    "                          validation rows, ranked on the device, macro-averaged over the n output columns that have both classes\n"
    "                          (up to 8 K >= 1; --ranks 1; not with --loss mse)\n"
    "            --weight-decay X   weight decay: L2 (added to the gradient) with --optimizer sgd | adam, decoupled with --optimizer adamw\n"
    "            --optimizer adamw  AdamW (beside sgd and adam)\n"
    "            --momentum M [--nesterov]   SGD momentum, 0 <= M < 1 (--optimizer sgd)\n"
    "            --clip-global T    clip the gradient by its norm over ALL parameters (torch's clip_grad_norm_), T > 0; --clip alone stays the\n"
    "                          per-group clip at 5\n"
    "            --no-decay-bias-norm   no weight decay on the biases and the norm parameters (b, gamma, beta, b1)\n"
    "            --fused-step       the epoch body is ONE call (gat_train_step: zero, forward, backward, clip, update), replayed as one launch\n"
    "                          on one rank; validation then comes from a forward of its own after the update\n"
    "                          (any of these flags runs the update on the device-side optimizer, gatv2_abi.h \"optimizer\": t and lr live there)\n"
    "            --ranks P [--transport rccl|host] [--halo 0|1|2]\n";

struct RankEnv {                      // one forked process per GPU
    int world = 1, rank = 0;
    struct Shared { volatile int id_ready; char id[GAT_COMM_ID_BYTES]; }* shared = nullptr;
    std::string shm_name;
    Prebuilt graph;                   // world > 1 with an edge-list dataset or graph flags
};

[[noreturn]] void die(const std::string& msg) {
    std::cerr << msg;
    std::exit(1);
}

bool split_ints(const std::string& csv, int count, std::vector<int32_t>& out) {
    out.clear();
    std::stringstream ss(csv);
    std::string item;
    for (int i = 0; i < count; ++i) {
        if (!std::getline(ss, item, ',')) return false;
        out.push_back(std::stoi(item));
    }
    return true;
}

// The reference scans argv three times (E:943-953, 958-1010, 1053-1061): --num-layers is looked
// up first so that --heads/--outdims can be sized; unknown flags are ignored.
Options parse_args(int argc, char** argv) {
    Options o;
    for (int i = 1; i + 1 < argc; ++i)
        if (std::string(argv[i]) == "--num-layers") {
            o.layers = std::stoi(argv[i + 1]);
            if (o.layers <= 0) die("Error: Number of layers must be > 0\n");
            break;
        }
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        const bool has_val = i + 1 < argc;
        if (a == "--epochs" && has_val) o.epochs = std::stoi(argv[++i]);
        else if (a == "--heads" && has_val) {
            if (!split_ints(argv[++i], o.layers, o.heads))
                die("Error: --heads must have " + std::to_string(o.layers) + " values.\n");
            o.heads_given = true;
        } else if (a == "--outdims" && has_val) {
            if (!split_ints(argv[++i], o.layers, o.outdims))
                die("Error: --ooutdims must have " + std::to_string(o.layers) + " values.\n");   // sic, E:982
            o.outdims_given = true;
        } else if (a == "--clip") o.clip = true;
        else if (a == "--optimizer" && has_val) {
            o.optimizer = argv[++i];
            if (o.optimizer != "sgd" && o.optimizer != "adam" && o.optimizer != "adamw") die("Invalid optimizer choice. Use 'sgd' or 'adam'\n");
        } else if (a == "--beta1" && has_val) { o.beta1 = std::stof(argv[++i]); o.beta1_given = true; }
        else if (a == "--beta2" && has_val) { o.beta2 = std::stof(argv[++i]); o.beta2_given = true; }
        else if (a == "--lr" && has_val) o.lr = std::stof(argv[++i]);
        else if (a == "--dataset" && has_val) o.dataset = argv[++i];
        else if (a == "--data-root" && has_val) o.data_root = argv[++i];
        else if (a == "--seed" && has_val) { o.seed = std::strtoull(argv[++i], nullptr, 0); o.seed_given = true; }
        else if (a == "--train-mask" && has_val) o.train_mask = argv[++i];
        else if (a == "--val-mask" && has_val) o.val_mask = argv[++i];
        else if (a == "--load-params" && has_val) o.load_params = argv[++i];
        else if (a == "--dump-params" && has_val) o.dump_params = argv[++i];
        else if (a == "--device" && has_val) o.device = std::stoi(argv[++i]);
        else if (a == "--cache") o.cache = true;
        else if (a == "--add-self-loops") o.graph_flags |= GAT_GRAPH_SELF_LOOPS;
        else if (a == "--undirected") o.graph_flags |= GAT_GRAPH_SYMMETRIZE;
        else if (a == "--coalesce") o.graph_flags |= GAT_GRAPH_COALESCE;
        else if (a == "--ranks" && has_val) {
            o.ranks = std::stoi(argv[++i]);
            if (o.ranks < 1) die("Error: --ranks must be >= 1\n");
        } else if (a == "--dtype" && has_val) {
            o.dtype = argv[++i];
            if (o.dtype != "f32" && o.dtype != "bf16") die("Invalid dtype choice. Use 'f32' or 'bf16'\n");
        } else if (a == "--halo" && has_val) {
            o.halo = std::stoi(argv[++i]);
            if (o.halo < 0 || o.halo > 2) die("Invalid halo choice. Use 0, 1 or 2\n");
        } else if (a == "--dropout" && has_val) o.dropout = std::strtof(argv[++i], nullptr);
        else if (a == "--attn-dropout" && has_val) o.attn_dropout = std::strtof(argv[++i], nullptr);
        else if (a == "--drop-edge" && has_val) o.drop_edge = std::strtof(argv[++i], nullptr);
        else if (a == "--drop-edge-keep-self") o.drop_edge_flags |= GAT_DROPEDGE_KEEP_SELF;
        else if (a == "--drop-edge-shared") o.drop_edge_flags |= GAT_DROPEDGE_SHARED_LAYERS;
        else if (a == "--residual") o.residual_flags |= GAT_RES_LINEAR;
        else if (a == "--bias") o.residual_flags |= GAT_RES_BIAS;
        else if (a == "--layer-norm") o.norm_flags |= GAT_NORM_LAYER;
        else if (a == "--batch-norm") o.batch_norm = true;
        else if (a == "--bn-momentum" && has_val) o.bn_momentum = std::strtof(argv[++i], nullptr);
        else if (a == "--norm-skip-last") o.norm_flags |= GAT_NORM_SKIP_LAST;
        else if (a == "--norm-eps" && has_val) o.norm_eps = std::strtof(argv[++i], nullptr);
        else if (a == "--edge-features") o.edge_features = true;
        else if (a == "--readout" && has_val) o.readout = argv[++i];
        else if (a == "--pairs" && has_val) o.pairs = argv[++i];
        else if (a == "--neg-sampling" && has_val) o.neg_sampling = argv[++i];
        else if (a == "--neg-first" && has_val) o.neg_first = std::strtoll(argv[++i], nullptr, 0);
        else if (a == "--neg-seed" && has_val) o.neg_seed = std::strtoull(argv[++i], nullptr, 0);
        else if (a == "--neg-both-directions") o.neg_flags |= GAT_NEG_BOTH_DIRECTIONS;
        else if (a == "--neg-allow-self") o.neg_flags |= GAT_NEG_ALLOW_SELF;
        else if (a == "--loss" && has_val) o.loss = argv[++i];
        else if (a == "--weight-decay" && has_val) o.weight_decay = std::strtof(argv[++i], nullptr);       // (the four values are checked in main)
        else if (a == "--momentum" && has_val) o.momentum = std::strtof(argv[++i], nullptr);
        else if (a == "--clip-global" && has_val) o.clip_global = std::strtof(argv[++i], nullptr);
        else if (a == "--nesterov") o.nesterov = true;
        else if (a == "--no-decay-bias-norm") o.no_decay_bias_norm = true;
        else if (a == "--fused-step") o.fused_step = true;
        else if (a == "--head-hidden" && has_val) o.head_hidden = std::atoi(argv[++i]);       // (checked in main, before anything touches the GPU)
        else if (a == "--head-act" && has_val) o.head_act = std::string(argv[++i]) == "lrelu" ? GAT_HEAD_ACT_LRELU : 0;
        else if (a == "--rank-metrics" && has_val) {          // (checked in main, before anything touches the GPU)
            o.rank_metrics = true;
            for (const char* p = argv[++i]; *p;) {
                char* end = nullptr;
                const long k = std::strtol(p, &end, 10);
                if (end == p) break;
                o.rank_ks.push_back((int32_t)k);
                p = *end == ',' ? end + 1 : end;
            }
        }
        else if (a == "--transport" && has_val) {
            o.transport = argv[++i];
            if (o.transport != "rccl" && o.transport != "host") die("Invalid transport choice. Use 'rccl' or 'host'\n");
        }
    }
    if (o.optimizer == "adam" || o.optimizer == "adamw") {
        if (o.beta1 <= 0.0f || o.beta1 >= 1.0f || o.beta2 <= 0.0f || o.beta2 >= 1.0f)
            die("Error: For Adam optimizer, beta1 and beta2 must be in (0,1).\n");
    } else if (o.beta1_given || o.beta2_given) {
        std::cerr << "Warning: beta1/beta2 specified but ignored for SGD optimizer.\n";
    }
    if (o.batch_norm && (o.norm_flags & GAT_NORM_LAYER)) die("Error: --batch-norm and --layer-norm exclude each other (one normaliser per model).\n");
    if (o.batch_norm && o.ranks > 1) die("Error: --batch-norm runs on one rank (the column statistics of a shard would need an exchange).\n");
    // The reference leaves head[]/out_dim[] uninitialised without these flags.
    if (!o.heads_given) die("Error: --heads must have " + std::to_string(o.layers) + " values.\n");
    if (!o.outdims_given) die("Error: --ooutdims must have " + std::to_string(o.layers) + " values.\n");
    const char* env_root = std::getenv("DATA_ROOT");             // E:1064-1067
    if (env_root && o.data_root == "./data") o.data_root = env_root;
    if (!o.data_root.empty() && o.data_root.back() != '/' && o.data_root.back() != '\\') o.data_root += '/';
    return o;
}

// ---- dataset text files (R:20-27; E:24-64) ----------------------------------------------------
// Whole-file read + strtof/strtol scanning: the reference's iostream loaders are the start-up
// bottleneck on large graphs; the accepted syntax (whitespace separated numbers) is the same.
bool slurp(const std::string& path, std::string& out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) { out.clear(); return false; }
    std::ostringstream ss;
    ss << f.rdbuf();
    out = ss.str();
    return true;
}

void load_features(const std::string& path, std::vector<float>& x, int64_t& n, int& dim) {
    std::string buf;
    slurp(path, buf);
    n = 0; dim = 0;
    const char* p = buf.c_str();
    const char* end = p + buf.size();
    while (p < end) {
        const char* eol = static_cast<const char*>(memchr(p, '\n', end - p));
        if (!eol) eol = end;
        int count = 0;
        const char* q = p;
        while (q < eol) {
            char* next = nullptr;
            const float v = std::strtof(q, &next);
            if (next == q || next > eol) break;
            x.push_back(v);
            ++count;
            q = next;
        }
        if (dim == 0) dim = count;
        else if (count != dim) {
            std::cerr << "Inconsistent input_dim on line " << n << std::endl;   // E:43
            std::exit(1);
        }
        ++n;
        p = eol + 1;
    }
}

void load_ints(const std::string& path, std::vector<int32_t>& v) {
    std::string buf;
    slurp(path, buf);
    const char* p = buf.c_str();
    for (;;) {
        char* next = nullptr;
        const long val = std::strtol(p, &next, 10);
        if (next == p) break;
        v.push_back((int32_t)val);
        p = next;
    }
}

bool file_exists(const std::string& p) { struct stat s{}; return stat(p.c_str(), &s) == 0; }
// edges.txt takes the place of row_ptr.txt / col_idx.txt when those are absent
bool edge_list_dataset(const std::string& dir) { return file_exists(dir + "edges.txt") && !file_exists(dir + "row_ptr.txt"); }

bool load_edges(const std::string& path, std::vector<int32_t>& src, std::vector<int32_t>& dst) {
    std::vector<int32_t> v;
    load_ints(path, v);
    if (v.size() % 2 != 0) { std::cerr << "Invalid edges.txt: odd number of values\n"; return false; }
    src.resize(v.size() / 2); dst.resize(v.size() / 2);
    for (size_t i = 0; i < src.size(); ++i) { src[i] = v[2 * i]; dst[i] = v[2 * i + 1]; }
    return true;
}
// rows = destinations, columns = sources (E:74-82)
bool csr_to_edges(const std::vector<int32_t>& rp, const std::vector<int32_t>& ci, int64_t n, std::vector<int32_t>& src,
                  std::vector<int32_t>& dst) {
    if (rp[0] != 0 || (int64_t)rp[n] != (int64_t)ci.size()) { std::cerr << "Invalid row_ptr: must start at 0 and end at the edge count\n"; return false; }
    for (int64_t i = 0; i < n; ++i) if (rp[i + 1] < rp[i]) { std::cerr << "Invalid row_ptr: not monotone\n"; return false; }
    src = ci; dst.resize(ci.size());
    for (int64_t i = 0; i < n; ++i) for (int32_t e = rp[i]; e < rp[i + 1]; ++e) dst[e] = (int32_t)i;
    return true;
}
// count, then fill (gat_graph_from_coo): rp [n + 1] and ci are sized by `room`, which gets the edge count
bool build_graph(const std::vector<int32_t>& src, const std::vector<int32_t>& dst, int64_t n, int flags, int device,
                 int32_t* (*room)(void*, int64_t), void* arg, int32_t* rp, int64_t* e_out) {
    int64_t e = 0;
    if (gat_graph_from_coo(src.data(), dst.data(), (int64_t)src.size(), n, n, 0, flags, nullptr, nullptr, 0, &e, device) != 0) return false;
    int32_t* ci = room(arg, e);
    if (!ci) return false;
    *e_out = e;
    return gat_graph_from_coo(src.data(), dst.data(), (int64_t)src.size(), n, n, 0, flags, rp, ci, e, &e, device) == 0;
}
void print_graph_build(int flags, int64_t n_in, int64_t e) {
    std::cout << "Graph build: add-self-loops=" << ((flags & GAT_GRAPH_SELF_LOOPS) ? 1 : 0) << " undirected="
              << ((flags & GAT_GRAPH_SYMMETRIZE) ? 1 : 0) << " coalesce=" << ((flags & GAT_GRAPH_COALESCE) ? 1 : 0) << ": " << n_in
              << " input edges -> " << e << " edges" << std::endl;
}

// ---- binary cache: magic, N, F, E, then the four arrays as raw little-endian data ----------------
constexpr uint64_t kCacheMagic = 0x3143564154414755ull;   // "UGATAVC1"
bool newer(const std::string& a, const std::string& b) {
    struct stat sa{}, sb{};
    if (stat(a.c_str(), &sa) != 0 || stat(b.c_str(), &sb) != 0) return false;
    return sa.st_mtime >= sb.st_mtime;
}
bool load_cache(const std::string& file, const std::string& dir, std::vector<float>& x, int64_t& n, int& f,
                std::vector<int32_t>& rp, std::vector<int32_t>& ci, std::vector<int32_t>& lab) {
    for (const char* t : {"features.txt", "row_ptr.txt", "col_idx.txt", "labels.txt"})
        if (!newer(file, dir + t)) return false;
    std::ifstream in(file, std::ios::binary);
    uint64_t h[4] = {0, 0, 0, 0};
    if (!in.read(reinterpret_cast<char*>(h), sizeof(h)) || h[0] != kCacheMagic) return false;
    n = (int64_t)h[1]; f = (int)h[2];
    x.resize((size_t)n * f); rp.resize(n + 1); ci.resize(h[3]); lab.resize(n);
    in.read(reinterpret_cast<char*>(x.data()), x.size() * sizeof(float));
    in.read(reinterpret_cast<char*>(rp.data()), rp.size() * sizeof(int32_t));
    in.read(reinterpret_cast<char*>(ci.data()), ci.size() * sizeof(int32_t));
    in.read(reinterpret_cast<char*>(lab.data()), lab.size() * sizeof(int32_t));
    return (bool)in;
}
void save_cache(const std::string& file, const std::vector<float>& x, int64_t n, int f, const std::vector<int32_t>& rp,
                const std::vector<int32_t>& ci, const std::vector<int32_t>& lab) {
    std::ofstream out(file, std::ios::binary);
    const uint64_t h[4] = {kCacheMagic, (uint64_t)n, (uint64_t)f, (uint64_t)ci.size()};
    out.write(reinterpret_cast<const char*>(h), sizeof(h));
    out.write(reinterpret_cast<const char*>(x.data()), x.size() * sizeof(float));
    out.write(reinterpret_cast<const char*>(rp.data()), rp.size() * sizeof(int32_t));
    out.write(reinterpret_cast<const char*>(ci.data()), ci.size() * sizeof(int32_t));
    out.write(reinterpret_cast<const char*>(lab.data()), lab.size() * sizeof(int32_t));
}

void check(int rc, const char* what) {
    if (rc != 0) {
        std::fprintf(stderr, "Error launching %s: %s\n", what, gat_last_error());   // style of E:1191 …, but fatal
        std::exit(1);
    }
}

// E:929-933.  The reference prints this block BEFORE it looks at argv (E:943), so its argument-error exits
// still show it; main() therefore calls it ahead of parse_args.  With --ranks P > 1 the parent must not touch
// the HIP runtime before forking, so there rank 0 prints it at the start of run() instead.
size_t g_free_before = 0;
bool g_tracker_printed = false;
void print_memory_tracker_before() {
    size_t total_mem = 0;
    if (gat_mem_info(&g_free_before, &total_mem) != 0)     // like the reference: report and go on (E:1189-1192)
        std::fprintf(stderr, "Error launching gat_mem_info: %s\n", gat_last_error());
    std::printf("\n[Memory Tracker] Before allocation:\n");
    std::printf("  Total GPU memory: %.2f MB\n", total_mem / (1024.0 * 1024.0));
    std::printf("  Free GPU memory : %.2f MB\n", g_free_before / (1024.0 * 1024.0));
    g_tracker_printed = true;
}

int run(const Options& o, const RankEnv& env) {
    if (!g_tracker_printed) print_memory_tracker_before();
    const size_t free_before = g_free_before;
    size_t total_mem = 0;

    const int L = o.layers;
    std::cout << "Configuration:\n"
              << "  Number of layers: " << L << "\n"
              << "  Epochs: " << o.epochs << "\n"
              << "  Attention heads: [";
    for (int l = 0; l < L; ++l) std::cout << o.heads[l] << (l < L - 1 ? ", " : "");
    std::cout << "]\n  Output dimensions: [";
    for (int l = 0; l < L; ++l) std::cout << o.outdims[l] << (l < L - 1 ? ", " : "");
    std::cout << "]\n"
              << "  Gradient clipping: " << (o.clip ? "true" : "false") << "\n"
              << "  Optimizer: " << o.optimizer << "\n"
              << "  Learning rate: " << o.lr << "\n\n";

    const std::string path = o.data_root + o.dataset + "/";
    std::cout << "Using dataset: " << o.dataset << std::endl;
    std::cout << "Dataset path: " << path << std::endl;

    std::vector<float> x;
    int64_t N = 0; int F0 = 0;
    std::vector<int32_t> row_ptr, col_idx, labels;
    // Optional binary cache of the parsed text files (additive: --cache).  Parsing features.txt is the
    // start-up bottleneck at Products scale (~2 GB of text); the cache is rewritten whenever a text
    // file is newer than it.
    const std::string cache = path + "gatv2_cache.bin";
    const int readout = o.readout == "mean" ? GAT_READOUT_MEAN : o.readout == "sum" ? GAT_READOUT_SUM : o.readout == "max" ? GAT_READOUT_MAX : GAT_READOUT_NONE;
    const bool edge_list = edge_list_dataset(path);
    const int loss_mode = o.loss == "bce" ? GAT_LOSS_BCE : o.loss == "mse" ? GAT_LOSS_MSE : GAT_LOSS_SOFTMAX_CE;
    const int pair_mode = o.pairs == "mul" ? GAT_PAIR_MUL : o.pairs == "add" ? GAT_PAIR_ADD : GAT_PAIR_NONE;
    const bool use_cache = o.cache && !readout && !pair_mode && loss_mode == GAT_LOSS_SOFTMAX_CE;       // (the cache holds labels)
    std::vector<float> targets;                 // --loss bce|mse: [rows][TC] in place of the labels
    int64_t t_rows = 0; int TC = 0;
    auto load_supervision = [&]() {
        if (loss_mode == GAT_LOSS_SOFTMAX_CE) { load_ints(path + "labels.txt", labels); return; }
        load_features(path + "targets.txt", targets, t_rows, TC);
        labels.assign((size_t)t_rows, 0);       // (one entry per head row: the length checks below apply to the targets alike)
    };
    const char* bad_length = loss_mode == GAT_LOSS_SOFTMAX_CE ? "Invalid labels length\n"
                                                              : "Invalid targets length: targets.txt must hold one row per node (per graph with --readout, per pair with --pairs)\n";
    std::vector<int32_t> e_src, e_dst;
    if (edge_list) {
        load_features(path + "features.txt", x, N, F0);
        if (!env.graph.row_ptr && !load_edges(path + "edges.txt", e_src, e_dst)) return 1;
        load_supervision();
        if (!readout && !pair_mode && (int64_t)labels.size() != N) { std::cerr << bad_length; return 1; }
    } else if (!(use_cache && load_cache(cache, path, x, N, F0, row_ptr, col_idx, labels))) {
        load_features(path + "features.txt", x, N, F0);
        load_ints(path + "row_ptr.txt", row_ptr);
        if ((int64_t)row_ptr.size() != N + 1) { std::cerr << "Invalid row_ptr length\n"; return 1; }
        load_ints(path + "col_idx.txt", col_idx);
        load_supervision();
        if (!readout && !pair_mode && (int64_t)labels.size() != N) { std::cerr << bad_length; return 1; }
        if (use_cache) save_cache(cache, x, N, F0, row_ptr, col_idx, labels);
    }
    if (loss_mode != GAT_LOSS_SOFTMAX_CE) {
        if (TC < 1 || (int64_t)targets.size() != t_rows * TC) { std::cerr << "Invalid targets.txt: expected rows of equal length\n"; return 1; }
        std::cout << "Loss: " << o.loss << " on " << TC << " target column(s)" << std::endl;
    }
    // --readout: the graphs' node ranges; labels.txt then holds one line per graph
    std::vector<int32_t> graph_ptr;
    if (readout) {
        load_ints(path + "graph_ptr.txt", graph_ptr);
        bool ok = graph_ptr.size() >= 2 && graph_ptr.front() == 0 && (int64_t)graph_ptr.back() == N;
        for (size_t i = 0; ok && i + 1 < graph_ptr.size(); ++i) ok = graph_ptr[i + 1] >= graph_ptr[i];
        if (!ok) { std::cerr << "Invalid graph_ptr.txt: expected G+1 non-decreasing integers from 0 to the node count\n"; return 1; }
        if (labels.size() + 1 != graph_ptr.size()) { std::cerr << bad_length; return 1; }
        std::cout << "Readout: " << o.readout << " over " << graph_ptr.size() - 1 << " graphs" << std::endl;
    }
    // --pairs: the node pairs; labels.txt / targets.txt then hold one line per pair
    std::vector<int32_t> pair_u, pair_v;
    if (pair_mode) {
        std::vector<int32_t> uv;
        load_ints(path + "pairs.txt", uv);
        bool ok = !uv.empty() && uv.size() % 2 == 0;
        for (size_t i = 0; ok && i < uv.size(); ++i) ok = uv[i] >= 0 && (int64_t)uv[i] < N;
        if (!ok) { std::cerr << "Invalid pairs.txt: expected lines \"u v\" of two node indices below the node count\n"; return 1; }
        for (size_t i = 0; i < uv.size(); i += 2) { pair_u.push_back(uv[i]); pair_v.push_back(uv[i + 1]); }
        if (labels.size() != pair_u.size()) { std::cerr << bad_length; return 1; }
        std::cout << "Pairs: " << o.pairs << " over " << pair_u.size() << " pairs" << std::endl;
    }
    // rows of the output head: pairs with --pairs, graphs with --readout, else nodes
    const int64_t NH = pair_mode ? (int64_t)pair_u.size() : readout ? (int64_t)graph_ptr.size() - 1 : N;
    if (env.graph.row_ptr) {                    // built before the ranks were forked
        if (env.graph.n != N) { std::cerr << "Invalid labels length\n"; return 1; }
        row_ptr.assign(env.graph.row_ptr, env.graph.row_ptr + N + 1);
        col_idx.assign(env.graph.col_idx, env.graph.col_idx + env.graph.e);
        print_graph_build(o.graph_flags, env.graph.n_in, env.graph.e);
    } else if (edge_list || o.graph_flags) {
        if (!edge_list && !csr_to_edges(row_ptr, col_idx, N, e_src, e_dst)) return 1;
        if (N <= 0) { std::cerr << "Invalid labels length\n"; return 1; }
        row_ptr.assign(N + 1, 0);
        int64_t e_built = 0;
        auto room = [](void* v, int64_t e) { auto* c = static_cast<std::vector<int32_t>*>(v); c->assign((size_t)std::max<int64_t>(e, 1), 0); return c->data(); };
        const bool ok = build_graph(e_src, e_dst, N, o.graph_flags, o.device, room, &col_idx, row_ptr.data(), &e_built);
        if (!ok) check(1, "gat_graph_from_coo");
        col_idx.resize((size_t)e_built);
        print_graph_build(o.graph_flags, (int64_t)e_src.size(), e_built);
        std::vector<int32_t>().swap(e_src); std::vector<int32_t>().swap(e_dst);
    }
    const int64_t E = (int64_t)col_idx.size();
    std::vector<float> ea;                      // --edge-features: [E][Fe], row j for CSR edge j
    int Fe = 0;
    if (o.edge_features) {
        if (edge_list)
            die("Error: --edge-features needs a CSR dataset (row_ptr.txt + col_idx.txt): edge_features.txt lists one row per CSR edge, and an "
                "edges.txt dataset is rebuilt into another order on the device\n");
        int64_t ne = 0;
        load_features(path + "edge_features.txt", ea, ne, Fe);
        if (ne != E || Fe < 1 || (int64_t)ea.size() != E * Fe) {
            std::cerr << "Invalid edge_features.txt: expected " << E << " lines of equal length, one per CSR edge\n";
            return 1;
        }
        if (Fe > GAT_EDGE_DIM_MAX) { std::cerr << "Invalid edge_features.txt: more than " << GAT_EDGE_DIM_MAX << " values per edge\n"; return 1; }
        std::cout << "Edge features: " << Fe << " per edge" << std::endl;
    }

    int max_degree = 0;
    for (int64_t i = 0; i < N; ++i) max_degree = std::max(max_degree, row_ptr[i + 1] - row_ptr[i]);
    std::cout << "Max degree = " << max_degree << std::endl;
    const int C = loss_mode != GAT_LOSS_SOFTMAX_CE ? TC : *std::max_element(labels.begin(), labels.end()) + 1;          // E:1106-1107
    std::cout << "Number of classes = " << C << std::endl;
    std::cout << "Graph loaded: " << N << " nodes, " << E << " edges, "
              << "input_feature_vector_dim = " << F0 << std::endl;

    // ---- the reference's buffer-size report (E:1153-1350), same formulas ----
    std::vector<int64_t> in_dim(L);
    in_dim[0] = F0;
    for (int l = 1; l < L; ++l) in_dim[l] = (int64_t)o.heads[l - 1] * o.outdims[l - 1];
    const size_t fsz = sizeof(float);
    std::printf("\nsize of input features : %zu MB\n", (size_t)(N * F0 * fsz) / (1024 * 1024));
    std::printf("\nsize of graph data (CSR,COO, labels) : %zu KB\n",
                (size_t)(((N + 1) + E + N + 2 * E) * sizeof(int)) / 1024);
    size_t total_out = 0, total_heads = 0, total_w = 0, total_a = 0, total_ig = 0;
    for (int l = 0; l < L; ++l) {
        total_out += (l == L - 1) ? (size_t)N * o.outdims[l] : (size_t)N * o.heads[l] * o.outdims[l];
        total_heads += o.heads[l];
        total_w += (size_t)o.heads[l] * o.outdims[l] * 2 * in_dim[l];
        total_a += (size_t)o.heads[l] * o.outdims[l];
        total_ig += (size_t)N * o.heads[l] * o.outdims[l] * fsz;
    }
    const int max_heads = *std::max_element(o.heads.begin(), o.heads.end());
    std::printf("\nTotal size of layer outputs(pre & post activation): %zu MB\n", (2 * total_out * fsz) / (1024 * 1024));
    std::printf("Total size of attention scores & coeffs: %zu MB\n", (2 * total_heads * E * fsz) / (1024 * 1024));
    std::printf("\nTotal size of parameters and their gradients: %zu MB\n",
                ((total_w + total_a + (size_t)C * o.outdims[L - 1]) * 2 * fsz) / (1024 * 1024));
    std::printf("\nloss and accuracy storage: %zu MB\n", ((size_t)N * (sizeof(float) + sizeof(int))) / (1024 * 1024));
    std::printf("Total size of intermediate gradients: %zu MB\n",
                ((total_ig + (size_t)max_heads * E * 2) * fsz) / (1024 * 1024));     // E:1350 (its 4x quirk kept)

    // ---- device context ----
    gat_config cfg{};
    cfg.num_layers = L; cfg.heads = o.heads.data(); cfg.outdims = o.outdims.data();
    cfg.in_dim = F0; cfg.num_classes = C; cfg.negative_slope = 0.01f; cfg.device = o.device;
    cfg.storage_dtype = o.dtype == "bf16" ? GAT_DTYPE_BF16 : GAT_DTYPE_F32;
    int n_devices = 0;
    check(gat_device_count(&n_devices), "gat_device_count");
    if (env.world > 1) {
        if (o.device + env.world <= n_devices) cfg.device = o.device + env.rank;      // one GPU per rank
        else if (o.transport == "rccl") die("Error: --ranks " + std::to_string(env.world) + " needs that many GPUs from --device on "
                                            "(RCCL cannot share a GPU between ranks); found " + std::to_string(n_devices) + "\n");
    }
    gat_ctx* ctx = nullptr;
    check(gat_create(&cfg, &ctx), "gat_create");
    // residual / bias: before anything sizes the packed buffers; every rank of --ranks runs this with the same options
    if (o.residual_flags) check(gat_set_residual(ctx, o.residual_flags), "gat_set_residual");
    if (o.batch_norm) check(gat_set_batch_norm(ctx, GAT_BN_ON | ((o.norm_flags & GAT_NORM_SKIP_LAST) ? GAT_BN_SKIP_LAST : 0), o.norm_eps, o.bn_momentum), "gat_set_batch_norm");
    else if (o.norm_flags) check(gat_set_norm(ctx, o.norm_flags, o.norm_eps), "gat_set_norm");
    if (o.edge_features) check(gat_set_edge_dim(ctx, Fe), "gat_set_edge_dim");
    if (loss_mode != GAT_LOSS_SOFTMAX_CE) check(gat_set_loss(ctx, loss_mode), "gat_set_loss");
    if (o.head_hidden > 0) check(gat_set_head_hidden(ctx, o.head_hidden, o.head_act), "gat_set_head_hidden");
    int64_t nW = 0, nA = 0, nWo = 0, nWres = 0, nB = 0, nLnG = 0, nLnB = 0, nWe = 0, nW1 = 0, nB1 = 0;
    gat_param_count(ctx, GAT_PARAM_HEAD_W, &nW1); gat_param_count(ctx, GAT_PARAM_HEAD_B, &nB1);   // 0 without --head-hidden
    gat_param_count(ctx, GAT_PARAM_WE, &nWe);                                                 // 0 without --edge-features
    gat_param_count(ctx, GAT_PARAM_W, &nW); gat_param_count(ctx, GAT_PARAM_A, &nA); gat_param_count(ctx, GAT_PARAM_WO, &nWo);
    gat_param_count(ctx, GAT_PARAM_WRES, &nWres); gat_param_count(ctx, GAT_PARAM_B, &nB);     // 0 without the flags
    gat_param_count(ctx, GAT_PARAM_LN_G, &nLnG); gat_param_count(ctx, GAT_PARAM_LN_B, &nLnB);
    const int64_t nBn = o.batch_norm ? nLnG : 0;      // floats of running_mean, and of running_var: behind the last group of a parameter file
    if (env.world == 1) {
        check(gat_set_graph(ctx, row_ptr.data(), col_idx.data(), N, E, N, 0), "csr_to_coo_kernel");
        check(gat_set_features(ctx, x.data(), N, F0), "gat_set_features");
        if (readout) check(gat_set_readout(ctx, readout, graph_ptr.data(), NH), "gat_set_readout");      // before the labels: they are per graph
        if (pair_mode) check(gat_set_pairs(ctx, pair_mode, pair_u.data(), pair_v.data(), NH), "gat_set_pairs");      // likewise: per pair
        if (loss_mode != GAT_LOSS_SOFTMAX_CE) check(gat_set_targets(ctx, targets.data(), NH, C), "gat_set_targets");
        else check(gat_set_labels(ctx, labels.data(), NH), "gat_set_labels");
        if (o.edge_features) check(gat_set_edge_features(ctx, ea.data(), E, Fe), "gat_set_edge_features");
    } else {
        // this rank's destination range; sources as rows of the padded [world][max_rows] table; the static
        // input features replicated for every table row (layer 0 then needs no exchange)
        if (env.world > N) die("Error: more ranks than graph rows\n");
        const gatshard::Plan plan = gatshard::make_plan(row_ptr.data(), N, env.world, env.rank);
        std::vector<int32_t> rp_l, ci_l;
        gatshard::local_csr(plan, row_ptr.data(), col_idx.data(), rp_l, ci_l);
        check(gat_set_graph(ctx, rp_l.data(), ci_l.data(), plan.n_rows(), (int64_t)ci_l.size(), plan.n_table(), plan.table_row0()),
              "csr_to_coo_kernel");
        {
            const std::vector<float> xt = gatshard::table_features(plan, x.data(), F0);
            check(gat_set_source_features(ctx, xt.data(), plan.n_table(), F0), "gat_set_source_features");
        }
        if (loss_mode != GAT_LOSS_SOFTMAX_CE) check(gat_set_targets(ctx, targets.data() + plan.row0() * C, plan.n_rows(), C), "gat_set_targets");   // the shard's own rows
        else check(gat_set_labels(ctx, labels.data() + plan.row0(), plan.n_rows()), "gat_set_labels");
        check(gat_set_shard_bounds(ctx, env.world, plan.bounds.data()), "gat_set_shard_bounds");     // dropout masks: unsharded node ids
        if (o.transport == "rccl") {
            if (env.rank == 0) {
                check(gat_comm_unique_id(env.shared->id), "gat_comm_unique_id");
                __sync_synchronize();
                env.shared->id_ready = 1;
            } else {
                while (!env.shared->id_ready) usleep(1000);
                __sync_synchronize();
            }
            check(gat_comm_init_rccl(ctx, env.world, env.rank, env.shared->id), "gat_comm_init_rccl");
        } else {
            int64_t hd_max = 0;
            for (int l = 0; l < L; ++l) hd_max = std::max<int64_t>(hd_max, (int64_t)o.heads[l] * o.outdims[l]);
            const int64_t bytes = std::max<int64_t>(plan.n_table() * hd_max + 64, nW + nA + nWo + nWres + nB + nLnG + nLnB + nWe + nW1 + nB1 + 3) * (int64_t)sizeof(float);   // (+ 64: block offsets of a halo exchange)
            check(gat_comm_init_host(ctx, env.world, env.rank, env.shm_name.c_str(), bytes), "gat_comm_init_host");
        }
        if (o.halo != 0) check(gat_comm_option(ctx, GAT_COMM_HALO, o.halo), "gat_comm_option(GAT_COMM_HALO)");      // collective: every rank
    }
    // the 4 GiB cliff of gatv2_abi.h "Limits" is never silent: ask every layer which kernels it runs on
    if (env.rank == 0) {
        std::string slow;
        for (int l = 0; l < L; ++l) {
            int32_t path = GAT_PATH_FAST;
            if (gat_layer_path(ctx, l, &path) == 0 && path == GAT_PATH_GENERIC_SIZE) slow += (slow.empty() ? "" : ", ") + std::to_string(l);
        }
        if (!slow.empty())
            fprintf(stderr, "Warning: layer(s) %s: the gathered source table is >= 4 GiB; these layers run on the generic float-atomic kernels "
                            "(same results, several times slower) — use --ranks to shard by destination range\n", slow.c_str());
    }
    // optional splits: loss / accuracy / gradient over the training nodes, an extra validation line per epoch
    std::vector<uint8_t> train_m, val_m;
    int64_t n_train = NH;
    auto load_mask = [&](const std::string& file, std::vector<uint8_t>& m, const char* what) {
        std::vector<int32_t> v;
        load_ints(file, v);
        if ((int64_t)v.size() != NH) die(std::string("Invalid ") + what + " length\n");
        m.resize((size_t)NH);
        for (int64_t i = 0; i < NH; ++i) m[(size_t)i] = v[(size_t)i] != 0;
    };
    if (!o.train_mask.empty()) {
        load_mask(o.train_mask, train_m, "train mask");
        n_train = 0;
        for (uint8_t b : train_m) n_train += b;
        if (n_train == 0) die("Error: --train-mask selects no node\n");
        const int64_t r0 = env.world == 1 ? 0 : gatshard::make_plan(row_ptr.data(), N, env.world, env.rank).row0();
        const int64_t nr = env.world == 1 ? NH : gatshard::make_plan(row_ptr.data(), N, env.world, env.rank).n_rows();
        check(gat_set_train_mask(ctx, train_m.data() + r0, nr), "gat_set_train_mask");
        std::printf("Training nodes: %lld of %lld\n", (long long)n_train, (long long)NH);
    }
    if (!o.val_mask.empty()) {
        if (env.world != 1) die("Error: --val-mask needs --ranks 1\n");
        load_mask(o.val_mask, val_m, "val mask");
    }
    // --loss bce|mse: the denominators are entry counts — the present targets of the training rows (all shards), and of the validation rows
    auto present = [&](const std::vector<uint8_t>& m) {
        int64_t cnt = 0;
        for (int64_t r = 0; r < NH; ++r) {
            if (!m.empty() && !m[(size_t)r]) continue;
            for (int c = 0; c < C; ++c) cnt += !std::isnan(targets[(size_t)(r * C + c)]);
        }
        return cnt;
    };
    const int64_t train_entries = loss_mode != GAT_LOSS_SOFTMAX_CE ? present(train_m) : 0;
    const int64_t val_entries = loss_mode != GAT_LOSS_SOFTMAX_CE && !val_m.empty() ? present(val_m) : 0;
    if (loss_mode != GAT_LOSS_SOFTMAX_CE) {
        if (train_entries == 0) die("Error: targets.txt has no present entry in the training rows\n");
        std::printf("Target entries: %lld present in the training rows\n", (long long)train_entries);
    }
    auto print_val = [&](double vl, int32_t vc, int32_t vn) {
        if (loss_mode == GAT_LOSS_SOFTMAX_CE) std::printf("Val Loss: %f, Val Accuracy: %.2f%%\n", vn ? vl / vn : 0.0, vn ? 100.0f * (static_cast<float>(vc) / vn) : 0.0f);
        else if (loss_mode == GAT_LOSS_BCE) std::printf("Val Loss: %f, Val Accuracy: %.2f%%\n", val_entries ? vl / val_entries : 0.0, val_entries ? 100.0f * (static_cast<float>(vc) / val_entries) : 0.0f);
        else std::printf("Val Loss: %f\n", val_entries ? vl / val_entries : 0.0);
    };
    // --rank-metrics: the ranking line behind a validation line (gat_eval_rank over the validation rows of the forward the validation
    // line came from): macro averages over the output columns that have both classes, and how many those are
    auto print_rank = [&]() {
        if (!o.rank_metrics) return;
        std::vector<gat_rank_stats> rs((size_t)C);
        check(gat_eval_rank(ctx, val_m.data(), NH, o.rank_ks.data(), (int32_t)o.rank_ks.size(), rs.data()), "gat_eval_rank");
        double auc = 0.0, ap = 0.0, mrr = 0.0;
        std::vector<double> hits(o.rank_ks.size(), 0.0);
        int n = 0;
        for (const gat_rank_stats& s : rs) {
            if (s.n_pos == 0 || s.n_neg == 0) continue;
            ++n;
            auc += (double)s.auc_num / (2.0 * (double)s.n_pos * (double)s.n_neg); ap += s.ap; mrr += s.mrr;
            for (size_t k = 0; k < hits.size(); ++k) hits[k] += (double)s.hits[k] / (double)s.n_pos;
        }
        const double d = n ? (double)n : 1.0;
        std::printf("Val AUC: %.6f, AP: %.6f, MRR: %.6f", auc / d, ap / d, mrr / d);
        for (size_t k = 0; k < hits.size(); ++k) std::printf(", Hits@%d: %.6f", (int)o.rank_ks[k], hits[k] / d);
        std::printf(" (%d column%s)\n", n, n == 1 ? "" : "s");
    };
    const bool dropout = o.dropout > 0.f || o.attn_dropout > 0.f || o.drop_edge > 0.f;
    const bool eval_pass = dropout || o.batch_norm || o.fused_step;   // validation needs a forward of its own in eval mode (--fused-step: the step leaves no forward to read)
    if (dropout) check(gat_set_dropout(ctx, o.dropout, o.attn_dropout, o.seed, 0), "gat_set_dropout");   // also seeds DropEdge
    if (o.drop_edge > 0.f) check(gat_set_dropedge(ctx, o.drop_edge, o.drop_edge_flags), "gat_set_dropedge");
    check(gat_params_init(ctx, o.seed), "xavier_init_kernel");
    if (!o.load_params.empty()) {
        std::vector<float> p(nW + nA + nWo + nWres + nB + nLnG + nLnB + nWe + nW1 + nB1 + 2 * nBn);    // the residual, norm, edge-feature and hidden-head groups follow the others, only with their flags
        std::ifstream f(o.load_params, std::ios::binary);
        if (!f.read(reinterpret_cast<char*>(p.data()), p.size() * sizeof(float))) die("Error: cannot read --load-params file\n");
        check(gat_params_set(ctx, GAT_PARAM_W, p.data(), nW), "gat_params_set");
        check(gat_params_set(ctx, GAT_PARAM_A, p.data() + nW, nA), "gat_params_set");
        check(gat_params_set(ctx, GAT_PARAM_WO, p.data() + nW + nA, nWo), "gat_params_set");
        if (nWres) check(gat_params_set(ctx, GAT_PARAM_WRES, p.data() + nW + nA + nWo, nWres), "gat_params_set");
        if (nB) check(gat_params_set(ctx, GAT_PARAM_B, p.data() + nW + nA + nWo + nWres, nB), "gat_params_set");
        if (nLnG) check(gat_params_set(ctx, GAT_PARAM_LN_G, p.data() + nW + nA + nWo + nWres + nB, nLnG), "gat_params_set");
        if (nLnB) check(gat_params_set(ctx, GAT_PARAM_LN_B, p.data() + nW + nA + nWo + nWres + nB + nLnG, nLnB), "gat_params_set");
        if (nWe) check(gat_params_set(ctx, GAT_PARAM_WE, p.data() + nW + nA + nWo + nWres + nB + nLnG + nLnB, nWe), "gat_params_set");
        if (nW1) check(gat_params_set(ctx, GAT_PARAM_HEAD_W, p.data() + nW + nA + nWo + nWres + nB + nLnG + nLnB + nWe, nW1), "gat_params_set");
        if (nB1) check(gat_params_set(ctx, GAT_PARAM_HEAD_B, p.data() + nW + nA + nWo + nWres + nB + nLnG + nLnB + nWe + nW1, nB1), "gat_params_set");
        if (nBn) {
            const float* stats = p.data() + (p.size() - 2 * nBn);
            check(gat_batch_norm_stats_set(ctx, GAT_BN_RUNNING_MEAN, stats, nBn), "gat_batch_norm_stats_set");
            check(gat_batch_norm_stats_set(ctx, GAT_BN_RUNNING_VAR, stats + nBn, nBn), "gat_batch_norm_stats_set");
        }
    }

    size_t free_after = 0;
    check(gat_mem_info(&free_after, &total_mem), "gat_mem_info");
    std::printf("\n[Memory Tracker] After all allocations:\n");
    std::printf("  Free GPU memory : %.2f MB\n", free_after / (1024.0 * 1024.0));
    std::printf("  Approx. GPU memory allocated by this program: %.2f MB\n",
                (double)(free_before - free_after) / (1024.0 * 1024.0));

    // --neg-sampling: lines neg_first .. of pairs.txt are the negative slots (their labels / targets stay those of the files)
    const int neg_mode = o.neg_sampling == "uniform" ? GAT_NEG_UNIFORM : o.neg_sampling == "corrupt" ? GAT_NEG_CORRUPT : GAT_NEG_NONE;
    if (neg_mode) {
        check(gat_set_negative_sampling(ctx, neg_mode, o.neg_first, NH - o.neg_first, o.neg_flags, o.neg_seed), "gat_set_negative_sampling");
        std::printf("Negative sampling: %s, pairs %lld .. %lld redrawn before every epoch\n", o.neg_sampling.c_str(), o.neg_first, (long long)NH - 1);
    }

    // any optimizer flag beyond the reference's: the update runs on the device-side optimizer (clip, decay and update in two launches)
    const bool dev_opt = o.device_optimizer();
    if (dev_opt) {
        gat_optimizer_config oc{};
        oc.kind = o.optimizer == "adamw" ? GAT_OPT_ADAMW : o.optimizer == "adam" ? GAT_OPT_ADAM : GAT_OPT_SGD;
        oc.flags = o.nesterov ? GAT_OPT_NESTEROV : 0;
        oc.lr = o.lr; oc.momentum = o.momentum; oc.beta1 = o.beta1; oc.beta2 = o.beta2; oc.eps = 1e-8f; oc.weight_decay = o.weight_decay;
        oc.decay_groups = 0xFFFFFFFFu;
        if (o.no_decay_bias_norm)
            oc.decay_groups = ((1u << (GAT_PARAM_HEAD_B + 1)) - 1u) & ~((1u << GAT_PARAM_B) | (1u << GAT_PARAM_NORM_G) | (1u << GAT_PARAM_NORM_B) | (1u << GAT_PARAM_HEAD_B));
        oc.clip_mode = o.clip_global > 0.f ? GAT_CLIP_GLOBAL : o.clip ? GAT_CLIP_PER_GROUP : GAT_CLIP_NONE;
        oc.clip_threshold = o.clip_global > 0.f ? o.clip_global : 5.0f;
        check(gat_set_optimizer(ctx, &oc), "gat_set_optimizer");
        if (o.fused_step && env.world == 1) check(gat_step_graph(ctx, 1), "gat_step_graph");
    }
    check(gat_zero_grad(ctx), "gat_zero_grad");
    for (int epoch = 1; epoch <= o.epochs; ++epoch) {
        const auto start = std::chrono::high_resolution_clock::now();
        std::printf("\nEpoch %d\n", epoch);
        if (neg_mode) {                           // fresh non-edges for this epoch, the first included
            check(gat_resample_negatives(ctx, (uint64_t)epoch), "gat_resample_negatives");
            int64_t unfiltered = 0;
            check(gat_negatives_info(ctx, nullptr, nullptr, nullptr, nullptr, &unfiltered), "gat_negatives_info");
            if (unfiltered) fprintf(stderr, "Warning: epoch %d: %lld negative(s) found no non-edge in %d attempts and are unfiltered\n", epoch, (long long)unfiltered, GAT_NEG_TRIES);
        }
        float loss_sum = 0.f; int32_t n_correct = 0;
        if (o.fused_step) check(gat_train_step(ctx, &loss_sum, &n_correct), "gat_train_step");
        else check(gat_forward(ctx, &loss_sum, &n_correct), "gatv2 forward");
        if (loss_mode == GAT_LOSS_SOFTMAX_CE) std::printf("\nAvg Loss: %f, Accuracy: %.2f%%\n", loss_sum / n_train, 100.0f * (static_cast<float>(n_correct) / n_train));
        else if (loss_mode == GAT_LOSS_BCE) std::printf("\nAvg Loss: %f, Accuracy: %.2f%%\n", loss_sum / train_entries, 100.0f * (static_cast<float>(n_correct) / train_entries));
        else std::printf("\nAvg Loss: %f\n", loss_sum / train_entries);
        if (!val_m.empty() && !eval_pass) {
            double vl = 0.0; int32_t vc = 0, vn = 0;
            check(gat_eval_mask(ctx, val_m.data(), NH, &vl, &vc, &vn), "gat_eval_mask");
            print_val(vl, vc, vn);
            print_rank();
        }
        if (!o.fused_step) {                      // (--fused-step: zero, forward, backward, clip and update were the one call above)
            check(gat_backward(ctx), "gatv2 backward");
            if (dev_opt) check(gat_optimizer_step(ctx), "gat_optimizer_step");      // clip, decay and update in two launches
            else {
                if (o.clip) check(gat_clip(ctx, 5.0f), "clip_grad_norm");           // E:1563
                if (o.optimizer == "adam") check(gat_step_adam(ctx, o.lr, o.beta1, o.beta2, 1e-8f, epoch), "adam_update_kernel");
                else check(gat_step_sgd(ctx, o.lr), "sgd_update_kernel");
            }
            check(gat_zero_grad(ctx), "gat_zero_grad");
        }
        if (!val_m.empty() && eval_pass) {        // validation of the updated model, without dropout, on the running statistics
            double vl = 0.0; int32_t vc = 0, vn = 0;
            check(gat_set_training(ctx, 0), "gat_set_training");
            check(gat_forward(ctx, nullptr, nullptr), "gatv2 forward");
            check(gat_eval_mask(ctx, val_m.data(), NH, &vl, &vc, &vn), "gat_eval_mask");
            check(gat_set_training(ctx, 1), "gat_set_training");
            print_val(vl, vc, vn);
            print_rank();
        }
        check(gat_sync(ctx), "gat_sync");
        const std::chrono::duration<double, std::milli> elapsed = std::chrono::high_resolution_clock::now() - start;
        std::cout << " total time: " << elapsed.count() << " ms" << std::endl;
    }

    if (!o.dump_params.empty() && env.rank == 0) {
        std::vector<float> p(nW + nA + nWo + nWres + nB + nLnG + nLnB + nWe + nW1 + nB1 + 2 * nBn);    // without --residual / --bias / --layer-norm / --batch-norm / --edge-features / --head-hidden: the format of always
        check(gat_params_get(ctx, GAT_PARAM_W, p.data(), nW), "gat_params_get");
        check(gat_params_get(ctx, GAT_PARAM_A, p.data() + nW, nA), "gat_params_get");
        check(gat_params_get(ctx, GAT_PARAM_WO, p.data() + nW + nA, nWo), "gat_params_get");
        if (nWres) check(gat_params_get(ctx, GAT_PARAM_WRES, p.data() + nW + nA + nWo, nWres), "gat_params_get");
        if (nB) check(gat_params_get(ctx, GAT_PARAM_B, p.data() + nW + nA + nWo + nWres, nB), "gat_params_get");
        if (nLnG) check(gat_params_get(ctx, GAT_PARAM_LN_G, p.data() + nW + nA + nWo + nWres + nB, nLnG), "gat_params_get");
        if (nLnB) check(gat_params_get(ctx, GAT_PARAM_LN_B, p.data() + nW + nA + nWo + nWres + nB + nLnG, nLnB), "gat_params_get");
        if (nWe) check(gat_params_get(ctx, GAT_PARAM_WE, p.data() + nW + nA + nWo + nWres + nB + nLnG + nLnB, nWe), "gat_params_get");
        if (nW1) check(gat_params_get(ctx, GAT_PARAM_HEAD_W, p.data() + nW + nA + nWo + nWres + nB + nLnG + nLnB + nWe, nW1), "gat_params_get");
        if (nB1) check(gat_params_get(ctx, GAT_PARAM_HEAD_B, p.data() + nW + nA + nWo + nWres + nB + nLnG + nLnB + nWe + nW1, nB1), "gat_params_get");
        if (nBn) {
            float* stats = p.data() + (p.size() - 2 * nBn);
            check(gat_batch_norm_stats_get(ctx, GAT_BN_RUNNING_MEAN, stats, nBn), "gat_batch_norm_stats_get");
            check(gat_batch_norm_stats_get(ctx, GAT_BN_RUNNING_VAR, stats + nBn, nBn), "gat_batch_norm_stats_get");
        }
        std::ofstream f(o.dump_params, std::ios::binary);
        f.write(reinterpret_cast<const char*>(p.data()), p.size() * sizeof(float));
    }
    gat_destroy(ctx);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    bool multi = false;                                    // --ranks P > 1: see print_memory_tracker_before
    for (int i = 1; i + 1 < argc; ++i)
        if (std::string(argv[i]) == "--ranks" && std::atoi(argv[i + 1]) > 1) multi = true;
    // dropout / DropEdge probabilities are checked before anything touches the GPU (NaN and trailing garbage included)
    for (int i = 1; i + 1 < argc; ++i) {
        const std::string a = argv[i];
        if (a != "--dropout" && a != "--attn-dropout" && a != "--drop-edge") continue;
        char* end = nullptr;
        const float p = std::strtof(argv[i + 1], &end);
        if (end == argv[i + 1] || *end != '\0' || !(p >= 0.f && p < 1.f)) die("Error: " + a + " must be in [0, 1)\n");
    }
    // --help, --edge-features with what it cannot be combined with, and graph flags without a graph to apply them to, end here: before
    // anything touches the GPU
    bool graph_flag = false, edge_feat_flag = false, readout_flag = false, targets_flag = false, pairs_flag = false;
    bool neg_flag = false, neg_corrupt = false; long long neg_first = -1;
    bool rank_flag = false, val_flag = false, mse_flag = false, hidden_flag = false;
    bool momentum_flag = false, momentum_pos = false, nesterov_flag = false; std::string optimizer_name = "sgd";
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--help") { std::cout << kUsage; return 0; }
        if (a == "--val-mask" && i + 1 < argc) val_flag = true;
        if (a == "--rank-metrics") {                       // 1 .. GAT_RANK_MAX_KS integers >= 1, comma separated, nothing else
            const std::string v = i + 1 < argc ? argv[i + 1] : "";
            int n = 0;
            bool ok = !v.empty();
            for (const char* p = v.c_str(); ok && *p;) {
                char* end = nullptr;
                const long k = std::strtol(p, &end, 10);
                ok = end != p && *p >= '0' && *p <= '9' && k >= 1 && k <= 2147483647L && (*end == '\0' || (*end == ',' && end[1] != '\0')) && ++n <= GAT_RANK_MAX_KS;
                p = *end == ',' ? end + 1 : end;
            }
            if (!ok) die("Error: --rank-metrics takes 1 to " + std::to_string(GAT_RANK_MAX_KS) + " comma-separated integers K >= 1\n");
            rank_flag = true;
        }
        if (a == "--readout") {
            const std::string v = i + 1 < argc ? argv[i + 1] : "";
            if (v != "mean" && v != "sum" && v != "max") die("Error: --readout must be mean, sum or max\n");
            readout_flag = true;
        }
        if (a == "--pairs") {
            const std::string v = i + 1 < argc ? argv[i + 1] : "";
            if (v != "mul" && v != "add") die("Error: --pairs must be mul or add\n");
            pairs_flag = true;
        }
        if (a == "--neg-sampling") {
            const std::string v = i + 1 < argc ? argv[i + 1] : "";
            if (v != "uniform" && v != "corrupt") die("Error: --neg-sampling must be uniform or corrupt\n");
            neg_flag = true; neg_corrupt = v == "corrupt";
        }
        if (a == "--neg-first" && i + 1 < argc) {
            char* end = nullptr;
            neg_first = std::strtoll(argv[i + 1], &end, 0);
            if (end == argv[i + 1] || *end != '\0' || neg_first < 0) die("Error: --neg-first must be a line index of pairs.txt (>= 0)\n");
        }
        if (a == "--add-self-loops" || a == "--undirected" || a == "--coalesce") graph_flag = true;
        if (a == "--edge-features") edge_feat_flag = true;
        if (a == "--head-hidden") {                        // a positive integer, nothing else
            const char* v = i + 1 < argc ? argv[i + 1] : "";
            char* end = nullptr;
            const long k = std::strtol(v, &end, 10);
            if (end == v || *end != '\0' || k < 1 || k > 2147483647L) die("Error: --head-hidden must be an integer K >= 1 (the hidden layer's width)\n");
            hidden_flag = true;
        }
        if (a == "--head-act") {
            const std::string v = i + 1 < argc ? argv[i + 1] : "";
            if (v != "relu" && v != "lrelu") die("Error: --head-act must be relu or lrelu\n");
        }
        if (a == "--weight-decay" || a == "--momentum" || a == "--clip-global") {      // one finite number in the flag's range, nothing else
            const char* v = i + 1 < argc ? argv[i + 1] : "";
            char* end = nullptr;
            const float x = std::strtof(v, &end);
            const bool parsed = end != v && *end == '\0' && std::isfinite(x);
            if (a == "--weight-decay" && !(parsed && x >= 0.f)) die(std::string("Error: --weight-decay must be a finite number >= 0\n") + kUsage);
            if (a == "--momentum" && !(parsed && x >= 0.f && x < 1.f)) die(std::string("Error: --momentum must be in [0, 1)\n") + kUsage);
            if (a == "--clip-global" && !(parsed && x > 0.f)) die(std::string("Error: --clip-global must be a finite number > 0\n") + kUsage);
            if (a == "--momentum") { momentum_flag = true; momentum_pos = x > 0.f; }
        }
        if (a == "--nesterov") nesterov_flag = true;
        if (a == "--optimizer" && i + 1 < argc) optimizer_name = argv[i + 1];
        if (a == "--loss") {
            const std::string v = i + 1 < argc ? argv[i + 1] : "";
            if (v != "softmax" && v != "bce" && v != "mse") die("Error: --loss must be softmax, bce or mse\n");
            targets_flag = v != "softmax";
            mse_flag = v == "mse";
        }
    }
    if (momentum_flag && momentum_pos && optimizer_name != "sgd") die(std::string("Error: --momentum needs --optimizer sgd\n") + kUsage);
    if (nesterov_flag && !(momentum_pos && optimizer_name == "sgd")) die(std::string("Error: --nesterov needs --optimizer sgd and --momentum M > 0\n") + kUsage);
    if (rank_flag && !val_flag) die("Error: --rank-metrics needs --val-mask: the ranking is over the validation rows\n");
    if (rank_flag && multi) die("Error: --rank-metrics needs --ranks 1: a ranking is global and cannot be summed over shards\n");
    if (rank_flag && mse_flag) die("Error: --rank-metrics cannot be combined with --loss mse: a regression target has no binary relevance\n");
    if (edge_feat_flag && graph_flag)
        die("Error: --edge-features cannot be combined with --add-self-loops / --undirected / --coalesce: they rebuild the graph, and the rows of "
            "edge_features.txt (one per CSR edge of the dataset) would no longer match its edges\n");
    if (edge_feat_flag && multi)
        die("Error: --edge-features needs --ranks 1: this program does not cut edge_features.txt into shards (the library does: "
            "gat_set_edge_features on every shard's own CSR)\n");
    if (readout_flag && multi)
        die("Error: --readout needs --ranks 1: a graph of the batch may straddle two destination-range shards\n");
    if (pairs_flag && multi)
        die("Error: --pairs needs --ranks 1: an endpoint of a pair may live on another destination-range shard\n");
    if (hidden_flag && multi)
        die("Error: --head-hidden needs --ranks 1: the hidden layer in front of the output head has no sharded form\n");
    if (pairs_flag && readout_flag)
        die("Error: --pairs cannot be combined with --readout: the output head has one kind of row\n");
    if (neg_flag && !pairs_flag) die("Error: --neg-sampling needs --pairs: the negatives are lines of pairs.txt\n");
    if (neg_flag && neg_first < 0) die("Error: --neg-sampling needs --neg-first K: lines K.. of pairs.txt are the negative slots\n");
    if (neg_flag && neg_corrupt && neg_first < 1) die("Error: --neg-sampling corrupt needs --neg-first >= 1: lines 0..K-1 of pairs.txt are its source pairs\n");
    if (graph_flag || readout_flag || targets_flag || pairs_flag) {
        std::string root = "./data", name = "pubmed";
        bool root_given = false;
        for (int i = 1; i + 1 < argc; ++i) {
            if (std::string(argv[i]) == "--data-root") { root = argv[i + 1]; root_given = true; }
            if (std::string(argv[i]) == "--dataset") name = argv[i + 1];
        }
        const char* env_root = std::getenv("DATA_ROOT");
        if (env_root && !root_given) root = env_root;
        if (!root.empty() && root.back() != '/' && root.back() != '\\') root += '/';
        const std::string dir = root + name + "/";
        if (readout_flag && !file_exists(dir + "graph_ptr.txt"))
            die("Error: --readout needs graph_ptr.txt (G+1 integers: the first node of every graph, then the node count) in " + dir + "\n");
        if (pairs_flag && !file_exists(dir + "pairs.txt"))
            die("Error: --pairs needs pairs.txt (one line \"u v\" per pair: two node indices) in " + dir + "\n");
        if (targets_flag && !file_exists(dir + "targets.txt"))
            die("Error: --loss bce / mse needs targets.txt (one row of C floats per node, per graph with --readout, per pair with --pairs; nan = missing) in " + dir + "\n");
        if (graph_flag && !file_exists(dir + "edges.txt") && !(file_exists(dir + "row_ptr.txt") && file_exists(dir + "col_idx.txt")))
            die("Error: --add-self-loops / --undirected / --coalesce need a graph: no edges.txt and no row_ptr.txt + col_idx.txt in " + dir + "\n");
    }
    if (!multi) print_memory_tracker_before();
    Options o = parse_args(argc, argv);
    if (!o.seed_given) { o.seed = (uint64_t)time(nullptr); o.seed_given = true; }     // E:1305; one seed for all ranks
    if (o.ranks == 1) return run(o, RankEnv{});
    // One process per GPU, forked before anything touches the HIP runtime.
    void* mem = mmap(nullptr, 4096, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
    if (mem == MAP_FAILED) die("Error: mmap failed\n");
    std::memset(mem, 0, 4096);
    RankEnv env;
    env.world = o.ranks;
    env.shared = static_cast<RankEnv::Shared*>(mem);
    env.shm_name = "/gatv2_" + std::to_string((long)getpid());
    // Edge-list dataset or graph flags: the whole graph is built ONCE, in a short-lived child (this process must not
    // touch the HIP runtime before it forks its ranks); the CSR comes back in anonymous shared memory the ranks inherit.
    const std::string dir = o.data_root + o.dataset + "/";
    if (edge_list_dataset(dir) || o.graph_flags) {
        std::vector<int32_t> src, dst, labels;
        if (o.loss == "softmax") load_ints(dir + "labels.txt", labels);
        else {                                  // the node count from targets.txt: one row per node
            std::vector<float> t; int64_t rows = 0; int tc = 0;
            load_features(dir + "targets.txt", t, rows, tc);
            labels.assign((size_t)rows, 0);
        }
        const int64_t N = (int64_t)labels.size();
        if (N <= 0) die("Invalid labels length\n");
        if (edge_list_dataset(dir)) {
            if (!load_edges(dir + "edges.txt", src, dst)) return 1;
        } else {
            std::vector<int32_t> rp, ci;
            load_ints(dir + "row_ptr.txt", rp);
            if ((int64_t)rp.size() != N + 1) die("Invalid row_ptr length\n");
            load_ints(dir + "col_idx.txt", ci);
            if (!csr_to_edges(rp, ci, N, src, dst)) return 1;
        }
        const int64_t n_in = (int64_t)src.size();
        const int64_t cap = n_in * ((o.graph_flags & GAT_GRAPH_SYMMETRIZE) ? 2 : 1) + ((o.graph_flags & GAT_GRAPH_SELF_LOOPS) ? N : 0);
        const size_t bytes = (size_t)(4 + N + 1 + std::max<int64_t>(cap, 1)) * sizeof(int32_t);
        void* g = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
        if (g == MAP_FAILED) die("Error: mmap failed\n");
        int64_t* e_out = static_cast<int64_t*>(g);                 // [0]: edge count, written by the child
        int32_t* rp_out = static_cast<int32_t*>(g) + 4;
        int32_t* ci_out = rp_out + N + 1;
        std::fflush(nullptr);
        const pid_t pid = fork();
        if (pid < 0) die("Error: fork failed\n");
        if (pid == 0) {
            struct Room { int32_t* ci; int64_t cap; } room{ci_out, cap};
            auto give = [](void* v, int64_t e) { auto* r = static_cast<Room*>(v); return e <= r->cap ? r->ci : nullptr; };
            const bool ok = build_graph(src, dst, N, o.graph_flags, o.device, give, &room, rp_out, e_out);
            if (!ok) std::fprintf(stderr, "Error launching gat_graph_from_coo: %s\n", gat_last_error());
            std::fflush(nullptr);
            std::_Exit(ok ? 0 : 1);
        }
        int status = 0;
        if (waitpid(pid, &status, 0) < 0 || !WIFEXITED(status) || WEXITSTATUS(status) != 0) return 1;
        env.graph.row_ptr = rp_out; env.graph.col_idx = ci_out; env.graph.n = N; env.graph.e = *e_out; env.graph.n_in = n_in;
    }
    std::fflush(nullptr);
    std::vector<pid_t> kids;
    for (int r = 0; r < o.ranks; ++r) {
        const pid_t pid = fork();
        if (pid < 0) die("Error: fork failed\n");
        if (pid == 0) {
            env.rank = r;
            if (r != 0 && !std::freopen("/dev/null", "w", stdout)) std::_Exit(1);      // rank 0 prints
            const int rc = run(o, env);
            std::fflush(nullptr);
            std::_Exit(rc);
        }
        kids.push_back(pid);
    }
    int rc = 0;
    for (size_t left = kids.size(); left > 0; --left) {
        int status = 0;
        const pid_t done = wait(&status);
        if (done < 0) break;
        const bool ok = WIFEXITED(status) && WEXITSTATUS(status) == 0;
        if (!ok && rc == 0) {           // a rank failed: the others would wait for it in an exchange
            rc = 1;
            for (pid_t k : kids) if (k != done) kill(k, SIGTERM);
        }
    }
    return rc;
}
