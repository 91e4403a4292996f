"""Stop sequences on the device (web-rwkv-gguf_amd/csrc/wrk_stopseq_dev.h) against the restatement in
tests/stopseq_ref.py: the row kernel (`Context.stop_sequences_advance`) bit for bit, and multi-token stops in `generate_stop` and
`generate_queue` of both runners.

The loops run on the `small` synthetic models (V = 1000).  Where a test needs known draws it scripts them with a forced-chain grammar
(`wrk.grammar_from_choices`, one choice per sequence behind a marker token, as tests/test_gpu_grammar.py::test_forced_chain): in the
state behind its marker a sequence has exactly one allowed token per step, whatever the pick.  Every comparison is exact: ids, lengths,
match words, tails, and the bits of states, logits rows, occurrence rows, mu and log-probs against the same call without stops run for
lengths[b] steps."""
import ctypes as C
import functools

import numpy as np
import pytest

import queue_ref as QR
import stopseq_cases as K
import stopseq_ref as Q
import test_gpu_stop as TS
import wrk
from oracle import synth

pytestmark = pytest.mark.gpu

MARK = 900                      # marker tokens of the scripted chains: 900 + the chain's index
SAMPLER = dict(temperature=[1.0, 0.8, 1.2, 0.9], top_p=[0.9, 1.0, 0.8, 0.95])
PEN = dict(presence=0.3, frequency=0.2, decay=0.996)
U32P = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def ctx():
    c = wrk.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def model(v6=False):
    return synth.make_v6_gguf(synth.V6_CONFIGS["small"], 42) if v6 else synth.make_v7_gguf(synth.CONFIGS["small"], 42)


def vocab(v6=False):
    return (synth.V6_CONFIGS if v6 else synth.CONFIGS)["small"].num_vocab


def chains(ctx, V, scripts):
    """(Grammar, start states): sequence i, started in starts[i], draws scripts[i] and then K.END forever."""
    cls, trans, start = wrk.grammar_from_choices(V, [[MARK + i] + list(s) for i, s in enumerate(scripts)], K.END)
    g = wrk.Grammar(ctx, V, cls, trans)
    return g, [g.walk(start, [MARK + i]) for i in range(len(scripts))]


class Session:
    """A runtime of B slots whose every call starts from zero states (and a zeroed occurrence table): kind greedy / sample (Mirostat, so
    that a mu is carried) / pen; every call goes through generate_stop, with log-probs."""

    def __init__(self, ctx, v6, B, kind):
        self.rt = wrk.Runtime(ctx, wrk.GgufReader(model(v6)), num_batch=B)
        self.V, self.B, self.kind = vocab(v6), B, kind
        self.occ = wrk.Occurrence(ctx, B, self.V) if kind == "pen" else None
        self.zero = np.zeros_like(self.rt.state_back(0))

    def kw(self):
        B = self.B
        if self.kind == "greedy":
            return {}
        kw = {k: [v[b % 4] for b in range(B)] for k, v in SAMPLER.items()} | {"seed": [11 + b for b in range(B)]}
        if self.kind == "sample":
            return kw | {"mirostat": (3.0, 0.1)}
        return kw | {"occurrence": self.occ} | PEN

    def reset(self):
        for b in range(self.B):
            self.rt.state_load(self.zero, b)
            if self.occ:
                self.occ.load(b)

    def call(self, first, steps, g=None, gs=None, mode=1, groups=1, seqs=None, ids=None, tail=None, reset=True):
        rt = self.rt
        if reset:
            self.reset()
        tok, lens, logits = rt.generate_stop(first, steps, [] if ids is None else ids, mode=mode, groups=groups, want_logits=True, poll_steps=4,
                                             logprobs=2, grammar=g, grammar_state=gs, stop_sequences=seqs, stop_tail=tail, **self.kw())
        cp = lambda a: None if a is None else np.array(a)
        return dict(tok=tok, lens=lens, logits=logits, state=[rt.state_back(b) for b in range(self.B)],
                    occ=[self.occ.back(b) for b in range(self.B)] if self.occ else None, mu=cp(rt.last_mirostat_mu),
                    gs=cp(rt.last_grammar_state), lp=rt.last_logprobs, match=cp(rt.last_stop_match), tail=cp(rt.last_stop_tail))

    def close(self):
        if self.occ:
            self.occ.close()
        self.rt.close()


def check_frozen(S, got, first, g, gs, mode, groups, plain):
    """tests/test_gpu_stop.py::check_against_plain for calls that carry a grammar, a mu and log-probs: everything sequence b leaves
    against the same call without stops that runs lengths[b] steps (one such call per distinct length)."""
    refs = {plain["tok"].shape[0]: plain}
    for b in range(S.B):
        n = int(got["lens"][b])
        assert np.array_equal(got["tok"][:n, b], plain["tok"][:n, b]), b
        if n not in refs:
            refs[n] = S.call(first, n, g, gs, mode, groups)
        ref = refs[n]
        assert ref["match"] is None and ref["tail"] is None
        assert np.array_equal(ref["tok"][:, b], got["tok"][:n, b]), b
        assert np.array_equal(bits(got["state"][b]), bits(ref["state"][b])), f"state of sequence {b} (length {n})"
        assert np.array_equal(bits(got["logits"][b]), bits(ref["logits"][b])), f"last logits of sequence {b} (length {n})"
        if S.occ:
            assert np.array_equal(bits(got["occ"][b][0]), bits(ref["occ"][b][0])) and np.array_equal(got["occ"][b][1], ref["occ"][b][1]), b
        if ref["mu"] is not None:
            assert bits(got["mu"])[b] == bits(ref["mu"])[b], f"mu of sequence {b}"
        if ref["gs"] is not None:
            assert int(got["gs"][b]) == int(ref["gs"][b]), f"grammar state of sequence {b}"
        for have, want in zip(got["lp"], ref["lp"]):
            assert np.array_equal(np.ascontiguousarray(have[:n, b]).view(np.uint32), np.ascontiguousarray(want[:n, b]).view(np.uint32)), b


# ----------------------------------------------------------------------------------------------------------------- 1. the row kernel
ALPHABET = [5, 400, 999]


@pytest.mark.parametrize("rows", [1, 3, 64, 65, 256])
def test_row_kernel_matches_the_restatement(ctx, rows):
    rng = np.random.default_rng(rows)
    matched = 0
    for nseq in (0, 1, 8):
        for L in (1, 2, 8):
            seqs = [[[ALPHABET[j] for j in rng.integers(0, 3, L)] for _ in range(nseq)] for _ in range(rows)]
            ids = [[ALPHABET[int(rng.integers(0, 3))]] if rng.random() < 0.25 else [] for _ in range(rows)]
            if rows >= 3:
                ids[1] = list(range(100, 100 + wrk.MAX_STOP_TOKENS - 1)) + [ALPHABET[0]]        # a full stop set
            tails = [Q.empty_tail() for _ in range(rows)]
            dev = None
            for step in range(32):
                y = [ALPHABET[j] for j in rng.integers(0, 3, rows)]
                want = [Q.step(tails[r], y[r], seqs[r], ids[r]) for r in range(rows)]
                match, dev = ctx.stop_sequences_advance(tails if dev is None else dev, y, seqs if nseq else [[] for _ in range(rows)], ids,
                                                        num_vocab=1000)
                tails = [t for _, t in want]
                assert match.tolist() == [m for m, _ in want], (nseq, L, step)
                assert dev.tolist() == tails, (nseq, L, step)
                matched += sum(m not in (Q.NONE, Q.TOKEN) for m, _ in want)
    assert rows < 64 or matched > 0


def test_row_kernel_hand_worked_cases(ctx):
    n = len(K.CASES)
    seqs, ids = [c[3] for c in K.CASES], [c[4] for c in K.CASES]
    tails, ended = None, {}
    for step in range(K.STEPS):
        match, tails = ctx.stop_sequences_advance(tails, [K.stream(i)[step] for i in range(n)], seqs, ids)
        for i in range(n):
            if match[i] != Q.NONE and i not in ended:
                ended[i] = (step + 1, int(match[i]), tails[i].tolist())
    for i in range(n):
        assert ended.get(i, (K.STEPS, Q.NONE))[:2] == K.CASES[i][5], K.NAMES[i]
        if i in ended:
            assert ended[i][2] == K.want_tail(i), K.NAMES[i]


# ----------------------------------------------------------------------------------------------------------------- 2. scripted streams
#           v6     mode B  groups eager engine kind
SCRIPTED = [(False, 1, 7, 1, None, None, "greedy"),
            (False, 1, 7, 1, None, None, "sample"),
            (False, 1, 7, 1, None, None, "pen"),
            (False, 0, 7, 1, None, None, "sample"),
            (False, 1, 1, 1, None, None, "greedy"),         # the batch-1 engine
            (False, 1, 1, 1, None, "0", "sample"),          # the five-launch layer
            (False, 1, 7, 1, "1", None, "pen"),             # WRK_NO_GRAPH=1
            (False, 1, 7, 2, None, None, "sample"),         # two lanes
            (False, 1, 7, 2, None, None, "pen"),
            (True, 1, 7, 1, None, None, "sample"),
            (True, 0, 7, 1, None, None, "pen"),
            (True, 1, 1, 1, None, None, "greedy")]


@pytest.mark.parametrize("v6,mode,B,groups,eager,engine,kind", SCRIPTED)
def test_scripted_streams(ctx, monkeypatch, v6, mode, B, groups, eager, engine, kind):
    if eager is not None:
        monkeypatch.setenv("WRK_NO_GRAPH", eager)
    if engine is not None:
        monkeypatch.setenv("WRK_ENGINE", engine)
    n = len(K.CASES)
    g, starts = chains(ctx, vocab(v6), [c[2] for c in K.CASES])
    S = Session(ctx, v6, B, kind)
    for which in ([list(range(n))] if B == n else [[i] for i in range(n)]):        # the seven cases as seven sequences, or each alone
        first = [K.CASES[i][1] for i in which]
        gs = [starts[i] for i in which]
        plain = S.call(first, K.STEPS, g, gs, mode, groups)
        assert plain["tok"].T.tolist() == [K.stream(i) for i in which]             # the script holds
        got = S.call(first, K.STEPS, g, gs, mode, groups, seqs=[K.CASES[i][3] for i in which], ids=[K.CASES[i][4] for i in which])
        assert got["lens"].tolist() == [K.CASES[i][5][0] for i in which]
        assert got["match"].tolist() == [K.CASES[i][5][1] for i in which]
        assert got["tail"].tolist() == [K.want_tail(i) for i in which]
        assert got["tok"].shape[0] <= K.STEPS
        check_frozen(S, got, first, g, gs, mode, groups, plain)
    S.close()
    g.close()


# ----------------------------------------------------------------------------------------------------------------- 3. unscripted
@pytest.mark.parametrize("v6", [False, True])
def test_sequences_cut_out_of_the_plain_output(ctx, v6):
    B, steps = 3, 20
    S = Session(ctx, v6, B, "sample")
    first = TS.first_tokens(B, S.V)
    plain = S.call(first, steps)
    tok = plain["tok"]
    spare = TS.unused_id(tok, S.V)
    seqs = [[tok[5:7, 0].tolist()], [tok[9:12, 1].tolist(), [spare, int(tok[3, 1])]], [[spare, spare], [int(tok[0, 2]), spare, int(tok[2, 2])]]]
    want_len, want_match, want_tail = Q.lengths(tok, seqs)
    print(f"lengths {want_len.tolist()} match {want_match.tolist()}")
    assert (want_len < steps).any() and (want_match == Q.NONE).any()                # one ends before the last step, one never ends
    got = S.call(first, steps, seqs=seqs)
    assert got["lens"].tolist() == want_len.tolist() and got["match"].tolist() == want_match.tolist()
    assert got["tail"].tolist() == want_tail.tolist()
    want_tok, *_ = Q.apply(tok, seqs, steps_run=got["tok"].shape[0])
    assert np.array_equal(got["tok"], want_tok)
    check_frozen(S, got, first, None, None, 1, 1, plain)
    S.close()


# ----------------------------------------------------------------------------------------------------------------- 4. tail carry
@pytest.mark.parametrize("v6", [False, True])
def test_a_sequence_that_straddles_two_calls(ctx, v6):
    i = K.NAMES.index("decoys")
    _, x0, script, seqs, _, want = K.CASES[i]
    g, starts = chains(ctx, vocab(v6), [script])
    S = Session(ctx, v6, 1, "greedy")
    single = S.call([x0], K.STEPS, g, starts, seqs=[seqs])
    assert (int(single["lens"][0]), int(single["match"][0])) == want
    a = S.call([x0], K.SPLIT, g, starts, seqs=[seqs])
    assert a["lens"].tolist() == [K.SPLIT] and a["match"].tolist() == [Q.NONE] and a["tail"].tolist() == [K.SPLIT_TAIL]
    state_a = a["state"][0]
    nxt = [int(a["tok"][K.SPLIT - 1, 0])]                           # the last draw is fed next
    rest = K.STEPS - K.SPLIT
    S.rt.state_load(state_a, 0)
    b = S.call(nxt, rest, g, a["gs"], seqs=[seqs], tail=a["tail"], reset=False)
    assert b["lens"].tolist() == [2] and b["match"].tolist() == [0]
    n = want[0]
    assert np.concatenate([a["tok"][:, 0], b["tok"][:2, 0]]).tolist() == single["tok"][:n, 0].tolist()
    assert np.array_equal(bits(b["state"][0]), bits(single["state"][0])) and b["tail"].tolist() == single["tail"].tolist()
    assert int(b["gs"][0]) == int(single["gs"][0])
    S.rt.state_load(state_a, 0)
    c = S.call(nxt, rest, g, a["gs"], seqs=[seqs], reset=False)      # without the tail the second call cannot see the beginning
    assert c["lens"].tolist() == [rest] and c["match"].tolist() == [Q.NONE]
    S.close()
    g.close()


# ----------------------------------------------------------------------------------------------------------------- 5. the queue
MAX_NEW = 6
#          prompt          stop sequences                              stop ids  want (length, reason, match)
REQUESTS = [([10],         [[101, 102]],                                 [],     (3, 1, 0)),
            ([40, 41],     [[40, 41]],                                   [],     (6, 2, Q.NONE)),       # the prompt is the stop sequence
            ([50, 51, 52], [[51, 52, 140], [52, 140], [141, 142]],       [],     (3, 1, 2)),            # a prompt ending a b, a reply starting c
            ([14],         [],                                           [162],  (3, 1, Q.TOKEN)),
            ([15, 16],     [[185]],                                      [],     (6, 1, 0)),            # a match on the last allowed draw
            ([17],         [],                                           [],     (6, 2, Q.NONE)),
            ([18, 19],     [[222, 223], [221, 222, 223]],                [223],  (4, 1, 1))]


def script(r):
    return list(range(100 + 20 * r, 100 + 20 * r + MAX_NEW))


def queue_case(B):
    """The requests with, for every request that takes a slot over, two more stop sequences split between the previous request's last
    reply tokens and its own first: (sequences per request, the schedule)."""
    R = len(REQUESTS)
    seqs = [[list(q) for q in r[1]] for r in REQUESTS]
    lens = [r[3][0] for r in REQUESTS]
    rows, needed = QR.schedule([len(r[0]) for r in REQUESTS], lens, B)
    traps = 0
    for r in range(R):
        before = [p for p in range(R) if rows[p]["slot"] == rows[r]["slot"] and rows[p]["start_step"] < rows[r]["start_step"]]
        if before:
            p = max(before, key=lambda q: rows[q]["start_step"])
            end = script(p)[:lens[p]]
            seqs[r] += [[end[-1], script(r)[0]], end[-2:] + [script(r)[0]]]
            traps += 1
    assert traps == R - B
    for r in range(R):                                              # the restatement agrees with the hand-worked column, traps included
        assert Q.reply(script(r), seqs[r], REQUESTS[r][2], MAX_NEW) == REQUESTS[r][3], r
    return seqs, rows, needed


@pytest.mark.parametrize("v6,mode,B,kind,pool", [(False, 1, 2, "greedy", False), (False, 1, 3, "sample", False), (False, 0, 3, "greedy", False),
                                                (False, 1, 2, "greedy", True), (True, 1, 3, "greedy", False), (True, 1, 2, "sample", True)])
def test_queue(ctx, v6, mode, B, kind, pool):
    R = len(REQUESTS)
    seqs, rows, needed = queue_case(B)
    g, starts = chains(ctx, vocab(v6), [script(r) for r in range(R)])
    S = Session(ctx, v6, B, kind)
    kw = {} if kind == "greedy" else dict(temperature=0.9, top_p=0.8, seed=list(range(R)))
    prompts, ids = [r[0] for r in REQUESTS], [r[2] for r in REQUESTS]
    pk = {}
    if pool:
        entries = wrk.StatePool(ctx, S.rt, R)
        pk = dict(pool=entries, save_state=list(range(R)))
    got, steps_run = S.rt.generate_queue(prompts, stop=ids, max_new=MAX_NEW, mode=mode, poll_steps=4, grammar=g, grammar_state=starts,
                                         stop_sequences=seqs, **kw, **pk)
    match = S.rt.last_stop_match
    assert match is not None and S.rt.last_stop_tail is None
    for r in range(R):
        t, why, slot, start = got[r]
        n, reason, m = REQUESTS[r][3]
        print(f"request {r}: slot {slot} start {start} reason {why} match {int(match[r]):#x} reply {t.tolist()}")
        assert t.tolist() == script(r)[:n] and why == reason and int(match[r]) == m, r
        assert (slot, start) == (rows[r]["slot"], rows[r]["start_step"]), r
    assert steps_run == QR.steps_run(needed, 4, sum(len(p) for p in prompts) + R * MAX_NEW)
    if pool:
        # a saved entry is the state generate_stop freezes for the same reply: the one-token prompts replayed in their own slots
        assert S.rt.last_queue_saved == [True] * R
        for r in (0, 3):
            slot = got[r][2]
            first, gs = [K.END] * B, [starts[r]] * B
            first[slot] = REQUESTS[r][0][0]
            sq, si = [[] for _ in range(B)], [[] for _ in range(B)]
            sq[slot], si[slot] = seqs[r], ids[r]
            S.reset()
            tok, lens = S.rt.generate_stop(first, MAX_NEW, si, mode=mode, grammar=g, grammar_state=gs, stop_sequences=sq,
                                           **({} if kind == "greedy" else dict(temperature=0.9, top_p=0.8, seed=[r] * B)))
            assert tok[:lens[slot], slot].tolist() == got[r][0].tolist() and int(S.rt.last_stop_match[slot]) == REQUESTS[r][3][2]
            assert np.array_equal(bits(entries.back(r)), bits(S.rt.state_back(slot))), f"entry of request {r}"
        entries.close()
    S.close()
    g.close()


def test_queue_without_sequences_reports_none(ctx):
    S = Session(ctx, False, 2, "greedy")
    S.rt.generate_queue([[10], [11, 12]], stop=[[5], []], max_new=3)
    assert S.rt.last_stop_match is None and S.rt.last_stop_tail is None
    S.close()


# ----------------------------------------------------------------------------------------------------------------- 6. programs
def test_one_program_serves_any_stop_sequences(ctx):
    V, B, steps = vocab(), 3, 16
    S = Session(ctx, False, B, "greedy")
    first = TS.first_tokens(B, V)
    S.reset()
    before, _ = S.rt.generate_greedy(first, steps, mode=1)
    spare = TS.unused_id(before, V)
    for seqs in ([[before[2:4, 0].tolist()], [], []], [[], [before[0:1, 1].tolist(), [spare]], [before[6:9, 2].tolist()]], [[], [], []]):
        got = S.call(first, steps, seqs=seqs)
        want_tok, want_len, want_match, want_tail = Q.apply(before, seqs, steps_run=got["tok"].shape[0])
        assert np.array_equal(got["tok"], want_tok) and got["lens"].tolist() == want_len.tolist()
        assert got["match"].tolist() == want_match.tolist() and got["tail"].tolist() == want_tail.tolist()
    S.reset()
    after, _ = S.rt.generate_greedy(first, steps, mode=1)
    assert np.array_equal(before, after) and S.rt.last_stop_match is None
    S.close()


@pytest.mark.parametrize("kind", ["greedy", "pen"])
def test_a_call_with_ids_only_is_the_call_it_was(ctx, kind):
    data, V, B, steps = TS.model("small"), TS.vocab("small"), 3, 16
    plain = TS.Run(ctx, data, V, B, kind, 1, 1, steps)
    stops = [[TS.new_at(plain.tokens, 0, 2)[1]], [], [TS.new_at(plain.tokens, 2, 6)[1]]]
    got = TS.Run(ctx, data, V, B, kind, 1, 1, steps, stop=stops, poll_steps=4)
    TS.check_against_plain(ctx, data, V, B, kind, 1, 1, steps, plain, got, stops)
    # the same stops as ids of a call with (empty) stop sequences: the same lengths, and the match words say TOKEN
    S = Session(ctx, False, B, kind)
    first = TS.first_tokens(B, V)
    free = S.call(first, steps)["tok"]
    stops = [[TS.new_at(free, 0, 2)[1]], [], [TS.new_at(free, 2, 6)[1]]]
    a = S.call(first, steps, ids=stops)
    assert a["match"] is None and a["tail"] is None
    b = S.call(first, steps, ids=stops, seqs=[])
    assert b["lens"].tolist() == a["lens"].tolist() and np.array_equal(a["tok"], b["tok"])
    assert b["match"].tolist() == [Q.TOKEN, Q.NONE, Q.TOKEN]
    for s in range(B):
        assert np.array_equal(bits(a["state"][s]), bits(b["state"][s])) and np.array_equal(bits(a["logits"][s]), bits(b["logits"][s]))
    S.close()


# ----------------------------------------------------------------------------------------------------------------- 7. argument errors
def u32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint32))


GOOD = dict(stop_seq_tokens=[1, 2, 3], stop_seq_offsets=[0, 2, 3], stop_seq_owners=[0, 1, 2])
EMPTY = wrk.STOP_TAIL_EMPTY


def bad_sequence_arrays(V):
    nine = dict(stop_seq_tokens=[1] * 9, stop_seq_offsets=list(range(10)), stop_seq_owners=[0, 9, 9])
    return [dict(GOOD, stop_seq_tokens=None), dict(GOOD, stop_seq_offsets=None), dict(GOOD, stop_seq_owners=None),     # only some given
            dict(GOOD, stop_seq_owners=[1, 1, 2]), dict(GOOD, stop_seq_owners=[0, 2, 1]),                              # owners: start, order
            dict(GOOD, stop_seq_offsets=[1, 2, 3]), dict(GOOD, stop_seq_offsets=[0, 2, 1]),                            # offsets: start, order
            nine,                                                                                                      # nine for one owner
            dict(GOOD, stop_seq_offsets=[0, 2, 2]),                                                                    # an empty sequence
            dict(stop_seq_tokens=[1] * 10, stop_seq_offsets=[0, 9, 10], stop_seq_owners=[0, 1, 2]),                    # nine ids
            dict(GOOD, stop_seq_tokens=[1, V, 3])]                                                                     # an id >= num_vocab


@pytest.mark.parametrize("v6", [False, True])
def test_bad_arguments_are_rejected_before_any_launch(ctx, v6):
    V, B, steps = vocab(v6), 2, 6
    S = Session(ctx, v6, B, "greedy")
    rt = S.rt
    rt.generate_greedy([3, 4], 5)                                   # a state that is not zero
    state = [rt.state_back(b) for b in range(B)]
    ft, out, lens, run = u32([3, 4]), np.zeros((steps, B), np.uint32), np.zeros(B, np.uint32), C.c_uint32()
    fn, mdl = (wrk.hip.wrk_v6_generate_stop, rt.model6) if v6 else (wrk.hip.wrk_v7_generate_stop, rt.model)
    qfn = wrk.hip.wrk_v6_generate_queue if v6 else wrk.hip.wrk_v7_generate_queue

    def fill(o, kw):
        o._keep = []
        for k, v in kw.items():
            if v is not None:
                o._keep.append(u32(v))
                setattr(o, k, o._keep[-1].ctypes.data_as(U32P))
        return o

    def call(**kw):
        return fn(ctx.h, mdl, rt.state, ft.ctypes.data_as(U32P), B, steps, C.byref(fill(wrk.GenerateOptions(), kw)), out.ctypes.data_as(U32P),
                  lens.ctypes.data_as(U32P), None, C.byref(run), None, 1)

    def qcall(**kw):
        o = fill(wrk.QueueOptions(), dict(prompt_tokens=[3, 4, 5], prompt_offsets=[0, 1, 3], max_new=[2, 2], **kw))
        o.num_requests, o.max_steps = 2, 8
        res = [np.zeros(4, np.uint32) for _ in range(5)]
        r = wrk.QueueResult(*(a.ctypes.data_as(U32P) for a in res), C.pointer(run))
        return qfn(ctx.h, mdl, rt.state, B, C.byref(o), C.byref(r), None, 1)

    tail_ok = [EMPTY] * 5 + [1, 2] + [EMPTY] * 7
    assert call(**GOOD, out_stop_match=[0, 0], stop_tail=tail_ok) == 0      # the well-formed call the bad ones are variations of
    for b in range(B):
        rt.state_load(state[b], b)
    bad = [call(**kw) for kw in bad_sequence_arrays(V)]
    bad += [call(out_stop_match=[0, 0]), call(stop_tail=tail_ok),                                   # outputs without the arrays
            call(**GOOD, stop_tail=[EMPTY] * 6 + [V] + [EMPTY] * 7),                                # neither EMPTY nor < num_vocab
            call(**GOOD, stop_tail=[EMPTY] * 5 + [1, EMPTY] + [EMPTY] * 7),                         # EMPTY after an id
            call(**GOOD, stop_tail=[EMPTY] * 7 + [2] + [EMPTY] * 6)]
    assert bad == [1] * len(bad), bad                               # WRK_E_ARG
    qbad = [qcall(**kw) for kw in bad_sequence_arrays(V)] + [qcall(out_stop_match=[0, 0])]
    assert qbad == [1] * len(qbad), qbad
    for b in range(B):
        assert np.array_equal(bits(rt.state_back(b)), bits(state[b])), b

    # the row entry point: the same array errors, and its own
    def rows(tails=None, tokens=(1, 2), match=True, V_=V, **kw):
        a = {k: (None if v is None else u32(v)) for k, v in dict(GOOD, **kw).items()}
        p = lambda x: None if x is None else x.ctypes.data_as(U32P)
        t = u32([EMPTY] * 14 if tails is None else tails)
        tk, m = u32(tokens), np.zeros(2, np.uint32)
        return wrk.hip.wrk_stop_sequences_advance(ctx.h, V_, 2, p(a["stop_seq_tokens"]), p(a["stop_seq_offsets"]), p(a["stop_seq_owners"]), None, None,
                                                  p(t), p(tk), p(m) if match else None)
    assert rows() == 0
    rbad = [rows(**{k: v for k, v in kw.items()}) for kw in bad_sequence_arrays(V)]
    rbad += [rows(tokens=(1, V)), rows(match=False), rows(tails=[EMPTY] * 6 + [V] + [EMPTY] * 7), rows(tails=[5, EMPTY] + [EMPTY] * 12)]
    assert rbad == [1] * len(rbad), rbad

    # what the Python layer refuses on its own, and the model after all of it
    with pytest.raises(ValueError):
        rt.generate_stop([3, 4], steps, [], stop_tail=[[1], [2]])
    with pytest.raises(wrk.WrkError):
        rt.generate_stop([3, 4], steps, [], stop_sequences=[[V]])
    with pytest.raises(wrk.WrkError):
        rt.generate_queue([[3], [4]], max_new=2, stop_sequences=[[V + 1, 2]])
    S.reset()
    tok, n = rt.generate_stop([3, 4], steps, [], stop_sequences=[[1, 2]])
    S.reset()
    plain, _ = rt.generate_greedy([3, 4], steps)
    want_tok, want_len, *_ = Q.apply(plain, [[[1, 2]], [[1, 2]]], steps_run=tok.shape[0])
    assert np.array_equal(tok, want_tok) and n.tolist() == want_len.tolist()
    S.close()
