"""approxQTeam for the GPU drop-in env: a forager that plays a fixed linear Q function and baselineTeam's home guard.

Behaviour to match (pinned stream-exactly by fixture G9, tests/test_gpu_approxq.py::test_bots_stream_exact, and value by
value by fixture G10): the reference team (agents/approxQTeam.py:28-110, 194-292, 299-406, TRAINING = False).  Its
offensive agent scores every legal action with four features of (state, action) -- a bias, the ghosts within one step of
the cell the action leads to, whether a pellet is eaten there unthreatened, the maze distance from there to the nearest
pellet over the board's area -- each divided by ten and weighted with fixed numbers, summed as Python floats in that
order.  It draws `random.random()` once per turn and explores (`random.choice` of the legal actions) below 0.1, otherwise
plays `random.choice` of the best actions; with at most two pellets left it walks to the legal successor nearest its
start cell (first minimum, no draw).  Its defensive agent is baselineTeam's guard, which here walks home with at most two
pellets left as well.

Like agents/baselineTeam.py this file is written against the pmx API: the Q features are read straight from the packed
state (no successor is generated for them); only the walk home asks the env for the real successors, in one GPU round
trip.  `approxq_action<I>` in csrc/pmx_step.hip is the same arithmetic in-kernel (PMX_ACTION_APPROXQ_OFFENSE).
"""
import random

from pmx.agents.baselineTeam import ReflexBot, _cells, _guard_score
from pmx.capture_agents import CaptureAgent
from pmx.game_state import DIR_CODE

_STEP = ((0, 1), (1, 0), (0, -1), (-1, 0), (0, 0))       # action code -> (dx, dy)
_EPSILON = 0.1
_HOME_AT = 2
_Q_WEIGHTS = {"bias": -9.280875042529367, "ghosts": -16.6612110039328, "eats": 11.127808437648863,
              "closest": -3.099192562140742}


class QForager(CaptureAgent):
    def registerInitialState(self, gameState):
        CaptureAgent.registerInitialState(self, gameState)
        lay = gameState._layout
        self.home = gameState.getInitialAgentPosition(self.index)
        self.width, self.height = lay.width, lay.height
        left_half = (1 << (lay.width // 2)) - 1
        self.prey_mask = (((1 << lay.width) - 1) & ~left_half) if self.red else left_half
        self.foes = self.getOpponents(gameState)

    def q_value(self, now, prey, code):
        x = int(now.pos[self.index][0]) + _STEP[code][0]
        y = int(now.pos[self.index][1]) + _STEP[code][1]
        near = sum(1 for f in self.foes
                   if not now.pac[f] and f not in self.unseen and abs(int(now.pos[f][0]) - x) + abs(int(now.pos[f][1]) - y) <= 1)
        q = 0
        q += (1.0 / 10.0) * _Q_WEIGHTS["bias"]
        q += (near / 10.0) * _Q_WEIGHTS["ghosts"]
        if not near and (x, y) in prey:
            q += (1.0 / 10.0) * _Q_WEIGHTS["eats"]
        steps = min((self.getMazeDistance((x, y), cell) for cell in prey), default=None)
        if steps is not None and steps < 2 ** 62:          # unreachable pellets do not count (the reference's search finds none)
            q += ((float(steps) / (self.width * self.height)) / 10.0) * _Q_WEIGHTS["closest"]
        return q

    def chooseAction(self, gameState):
        now = gameState._state
        names = gameState.getLegalActions(self.index)                      # reference list order: N, S, E, W, Stop
        prey = set(_cells(now.food, self.height, self.prey_mask))
        self.unseen = [f for f in self.foes if gameState.getAgentPosition(f) is None]     # hidden by makeObservation, if asked on one
        if len(prey) <= _HOME_AT:
            options = gameState._engine.successors(now, self.index)        # all five successors, one GPU round trip
            best_name, best_d = None, 9999
            for name in names:
                nxt = options[DIR_CODE[name]][0]
                d = self.getMazeDistance(self.home, (int(nxt.pos[self.index][0]), int(nxt.pos[self.index][1])))
                if d < best_d:
                    best_name, best_d = name, d
            return best_name
        if random.random() < _EPSILON:
            return random.choice(names)
        marks = [self.q_value(now, prey, DIR_CODE[name]) for name in names]
        top = max(marks)
        return random.choice([name for name, m in zip(names, marks) if m == top])


def _forager(index):
    return QForager(index)


def _guard(index):
    return ReflexBot(index, _guard_score, home_at=_HOME_AT)


_ROLES = {"ApproxQLearningOffense": _forager, "DefensiveReflexAgent": _guard}


def createTeam(firstIndex, secondIndex, isRed, first="ApproxQLearningOffense", second="DefensiveReflexAgent", **args):
    return [_ROLES[first](firstIndex), _ROLES[second](secondIndex)]
